"""scratch/ab/block_compare.py <parent all.s> <new all.s> <kernel substring> [min block length]: the basic blocks of one kernel in two
disassemblies (scratch/ab/disasm.sh <object> writes /tmp/disasm/all.s), compared as multisets.  A block starts at the kernel's entry,
at a branch target and behind a branch; it is compared (a) as its full instruction text, registers and literals included, and (b) as
its sequence of mnemonics (the same instructions in the same order, registers free).  Prints the counts and every block of at least
<min block length> instructions (default 1) that one side has and the other has not, with its length and its memory / LDS /
transcendental mnemonic counts, so that the loops of a kernel are easy to find among them."""
import collections
import re
import sys


def blocks(path, key):
    ins, base, on = [], None, False
    for line in open(path):
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", line.strip())
        if m:
            if on:
                break
            if key in m.group(2):
                on, base = True, int(m.group(1), 16)
            continue
        if on and line.strip():
            text, _, tail = line.partition("//")
            a = re.match(r"\s*([0-9A-Fa-f]+):", tail)
            if not a:  # (padding and data words behind the code carry no instruction address)
                continue
            t = re.search(r"<[^>]*\+0x([0-9a-f]+)>", tail)
            ins.append((int(a.group(1), 16) - base, " ".join(text.split()), int(t.group(1), 16) if t else None))
    last = max(i for i, x in enumerate(ins) if x[1].startswith("s_endpgm"))
    ins = ins[:last + 1]
    leaders = {0}
    for i, (addr, text, target) in enumerate(ins):
        if re.match(r"s_(c?branch|endpgm|setpc)", text):
            if i + 1 < len(ins):
                leaders.add(ins[i + 1][0])
            if target is not None:
                leaders.add(target)
    out, cur = [], []
    for addr, text, target in ins:
        if addr in leaders and cur:
            out.append(cur); cur = []
        cur.append(re.sub(r"^(s_c?branch\S*) .*", r"\1", text))  # a branch's distance is not part of its block
    out.append(cur)
    return out, len(ins)


def main():
    key, least = sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 1
    (pb, pn), (nb, nn) = blocks(sys.argv[1], key), blocks(sys.argv[2], key)
    print(f"{key}: parent {pn} instructions in {len(pb)} blocks, new {nn} in {len(nb)}")
    for what, f in (("full text", lambda b: "\n".join(b)), ("mnemonic sequence", lambda b: " ".join(x.split()[0] for x in b))):
        cp, cn = collections.Counter(map(f, pb)), collections.Counter(map(f, nb))
        both = sum((cp & cn).values())
        print(f"  {what}: {both} blocks in both ({sum(len(k.split(chr(10) if what == 'full text' else ' ')) * v for k, v in (cp & cn).items())} instructions), "
              f"{sum((cp - cn).values())} only in the parent, {sum((cn - cp).values())} only in the new")
        if what == "mnemonic sequence":
            for side, d in (("parent only", cp - cn), ("new only", cn - cp)):
                for k, v in d.items():
                    ms = k.split()
                    if len(ms) >= least:
                        c = collections.Counter(ms)
                        print(f"    {side} x{v}: {len(ms)} instructions, global/buffer {sum(v2 for m, v2 in c.items() if m.startswith(('global_', 'buffer_', 'scratch_')))}, "
                              f"ds {sum(v2 for m, v2 in c.items() if m.startswith('ds_'))}, exp/rcp {c['v_exp_f32_e32'] + c['v_rcp_f32_e32']}, starts {' '.join(ms[:4])}")


main()
