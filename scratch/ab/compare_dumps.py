"""scratch/ab/compare_dumps.py DIR_A DIR_B: the arrays two `bench.py --dump-outputs` runs wrote, compared byte for byte
(ndarray.tobytes(): the sign of a zero and the payload of a NaN count).  Exit status 1 if any array differs or is missing."""
import os
import sys

import numpy as np

a_dir, b_dir = sys.argv[1], sys.argv[2]
names = sorted(f for f in os.listdir(a_dir) if f.endswith(".npy"))
bad = sorted(set(f for f in os.listdir(b_dir) if f.endswith(".npy")) ^ set(names))
for f in names:
    if f in bad:
        continue
    x, y = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
    same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    if same:
        diff, n = 0.0, 0
    else:
        bad.append(f)
        fin = np.isfinite(x) & np.isfinite(y) if x.shape == y.shape else None
        diff = float(np.abs(x[fin] - y[fin]).max() / max(float(np.abs(x[fin]).max()), 1e-30)) if fin is not None and fin.any() else float("nan")
        n = int((x != y).sum()) if x.shape == y.shape else -1
    print(f"{a_dir} vs {b_dir} {f}: {'BITWISE EQUAL' if same else 'DIFFERENT'} (max |x - y| / max |x| = {diff:.3e}; elements with x != y: {n}, "
          f"nonfinite {int((~np.isfinite(x)).sum())}, size {x.size})")
for f in bad:
    if f not in names or not os.path.exists(os.path.join(b_dir, f)):
        print(f"{f}: in one directory only")
sys.exit(1 if bad else 0)
