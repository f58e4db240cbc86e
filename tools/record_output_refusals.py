"""Records tests/golden/output_refusals_parent.json: what every call of the script of tests/test_gpu_output_refusals.py answers on
the library that is loaded (RDYHIP_LIB names another build of the same ABI), for that test to compare later builds with, message
for message and bit for bit.

    RDYHIP_LIB=/path/to/the/parent/librdyhip.so python tools/record_output_refusals.py [out_file]

Run once, on a GPU, against the commit BEFORE the output calls of the three states were folded into shared helpers.  Stored per
numbering: of every call its name, the return code and rdyhip_last_error(), of the successful ones their numbers as hex (results
of more than 32 values: the SHA-256 of that hex text), in the packed form of the test's dump_golden."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv):
    import test_gpu_output_refusals as T
    from rdycore_amd import build
    out = argv[0] if argv else T.GOLDEN
    print("library:", build.lib_path())
    golden = {numbering: T.run_script(numbering)[0] for numbering in T.NUMBERINGS}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(T.dump_golden(golden))
    for numbering, log in golden.items():
        print(f"{numbering}: {len(log)} calls, {sum(1 for r in log if r['rc'])} refused, {sum(1 for r in log if 'result' in r)} with numbers")
    print(f"-> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
