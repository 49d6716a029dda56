#!/bin/bash
# usage: disasm.sh <object or lib> [kernel-substring] -> /tmp/disasm/all.s (and /tmp/disasm/<substring>.s for the first kernel that matches)
# (pass the translation unit's object file, fresnel_amd/_lib/obj/<unit>.o: a .so holds one fat binary per unit and only the first is read)
#        disasm.sh --kernels <object> [<object> ...] -> one line per kernel of the objects' gfx950 code, sorted by name:
#   name (anonymous-namespace component removed), instruction count, sha256 of the instruction text (up to the last s_endpgm:
#   padding behind it, addresses and encodings do not count), then vgpr sgpr agpr lds scratch sgpr_spill vgpr_spill max_wg
#   from the code object's notes.  Two builds generate the same code for a kernel iff their lines are equal.
bin=/opt/rocm/lib/llvm/bin
tmp=/tmp/disasm; mkdir -p $tmp
unbundle() {
  $bin/llvm-objcopy --dump-section .hip_fatbin=$tmp/fat.bin $1 && \
  $bin/clang-offload-bundler --unbundle --type=o --input=$tmp/fat.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/dev.co
}
if [ "$1" = "--kernels" ]; then
  shift
  for obj in "$@"; do
    unbundle $obj || exit 1
    $bin/llvm-readelf --notes $tmp/dev.co | awk '
      $1 == "-" && $2 == ".agpr_count:" { a = $3 }
      $1 == ".group_segment_fixed_size:" { l = $2 } $1 == ".max_flat_workgroup_size:" { m = $2 } $1 == ".name:" { n = $2 }
      $1 == ".private_segment_fixed_size:" { p = $2 } $1 == ".sgpr_count:" { s = $2 } $1 == ".sgpr_spill_count:" { ss = $2 }
      $1 == ".vgpr_count:" { v = $2 } $1 == ".vgpr_spill_count:" { print n, v, s, a, l, p, ss, $2, m }' > $tmp/meta.txt
    rm -f $tmp/k_*.txt
    # per symbol, the text up to its last s_endpgm: lines are held back and appended to the symbol's file at every s_endpgm
    $bin/llvm-objdump -d --no-show-raw-insn --no-leading-addr $tmp/dev.co | awk -v dir=$tmp '
      /^<.*>:$/ { name = substr($0, 2, length($0) - 3); n = 0; next }
      name != "" && NF { sub(/[ \t]*\/\/.*$/, ""); line[++n] = $0
                         if ($1 == "s_endpgm") { f = dir "/k_" name ".txt"; for (i = 1; i <= n; ++i) print line[i] >> f; close(f); n = 0 } }' || exit 1
    while read name v s a l p ss vs m; do
      f=$tmp/k_$name.txt
      echo "$(echo $name | sed 's/12_GLOBAL__N_1//') insns=$(wc -l < $f) sha=$(sha256sum < $f | cut -c1-16) vgpr=$v sgpr=$s agpr=$a lds=$l scratch=$p sgpr_spill=$ss vgpr_spill=$vs max_wg=$m"
      rm -f $f
    done < $tmp/meta.txt
  done | sort
  exit 0
fi
obj=$1; k=$2
unbundle $obj || exit 1
$bin/llvm-objdump -d --no-show-raw-insn $tmp/dev.co > $tmp/all.s
if [ -n "$k" ]; then
  awk -v k="$k" '/^[0-9a-f]+ <.*>:/{f = index($0, k) > 0 && !done} f{print} /s_endpgm/{if (f) {done = 1; f = 0}}' $tmp/all.s > $tmp/$k.s
  wc -l $tmp/$k.s
fi
