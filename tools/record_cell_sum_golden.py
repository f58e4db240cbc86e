"""Records tests/golden/cell_sum_parent/*.npz: the results of the groups of tests/test_gpu_cell_sum_batch.py on the library
that is loaded (RDYHIP_LIB names another build of the same ABI), for that test to compare later builds with bit for bit.

    RDYHIP_LIB=/path/to/the/parent/librdyhip.so python tools/record_cell_sum_golden.py [out_dir]

Run once, on a GPU, against the commit BEFORE the batched cell sum.  Stored per evaluation: the SHA-256 of F, u_out, pv and
fdiv (the arrays themselves up to 256 rows) and the Courant struct."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv):
    import test_gpu_cell_sum_batch as T
    from rdycore_amd import build
    out_dir = argv[0] if argv else T.GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    os.environ["RDYHIP_KERNEL"] = "tiled"
    print("library:", build.lib_path())
    for group in T.GROUPS:
        results = T.run_group(group, T.OsEnv())
        for key, (name, call, res) in results.items():
            T.check_oracle(name, call, res, key)           # the recorded bits are the oracle's values too
        path = os.path.join(out_dir, group + ".npz")
        np.savez_compressed(path, **T.golden_arrays(results))
        print(f"{group}: {len(results)} evaluations -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
