"""The rows of tests/dispatch_table.py as the case lines tools/micro/launch_record.hip reads.
  python launch_record_cases.py            prints the rows of CASES
  python launch_record_cases.py RECORDER   runs RECORDER on CASES and, the knobs being read once per process, once per knob
                                           set of KNOB_CASES with that environment; prints every record"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
from dispatch_table import CASES, KNOB_CASES  # noqa: E402

LAYOUT = {"full6": 6, "pair5": 5, "elec3": 3, "pack2": 2, "sym8": 8}


def line(c):
    pairs = c["pairs"] or []
    return " ".join(str(v) for v in (c["id"], c["n"], c["T"], c["A"], c["G"], LAYOUT[c["layout"]], int(c["packed"]),
                                     int(c["energy_only"]), int(c["warm"]), c["nroots"], c["api"], int(c["keep"]),
                                     len(pairs), *[i for p in pairs for i in p]))


if len(sys.argv) < 2:
    print("\n".join(line(c) for c in CASES))
else:
    runs = [({}, CASES)] + [(c["env"], [c]) for c in KNOB_CASES]
    for env, cases in runs:
        print("ENV", " ".join(f"{k}={v}" for k, v in sorted(env.items())), flush=True)
        subprocess.run([sys.argv[1]], input="\n".join(line(c) for c in cases) + "\n", text=True, check=True,
                       env={**os.environ, **env})
