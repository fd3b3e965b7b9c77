"""Records tests/golden/trdm_plan.json from a source tree:  python make_trdm_plan.py TREE DISPATCH_RECORD
TREE: a checkout with its library built (python TREE/evcont_amd/build.py); DISPATCH_RECORD: tools/micro/dispatch_record.hip
compiled against the same tree.  The committed file comes from the last commit before csrc/gemv_dispatch.hip."""
import ctypes as C, json, os, subprocess, sys
TREE, RECORDER = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
sys.path.insert(0, TREE)
from evcont_amd import _lib
from evcont_amd._lib import TrdmSet
LAYOUT = {"full6": 6, "pair5": 5, "elec3": 3, "pack2": 2, "sym8": 8}
def shape(n, T, layout):
    n2, ns = n * n, n * (n + 1) // 2
    cols = ns * (ns + 1) // 2 if layout == "sym8" else (n2 * (n2 + 1) // 2 if layout in ("elec3", "pack2") else n2 * n2)
    rows = T * (T + 1) // 2 if layout in ("pair5", "pack2", "sym8") else T * T
    return rows, cols, (cols + 15) // 16 * 16, (n2 + 1) // 2 * 2
GS = [1, 2, 3, 4, 8, 9, 11, 12, 16, 17, 32, 33, 44, 64, 65, 76, 96]
# (n, T, layout, rows2 or None = all rows): H30 / T=20, the narrow shape, a tall one-body problem in an LDS launch of its
# own (Zundel, T=100), and one falling back to the fragment-shaped kernel (a shard of 3500 rows of T=118)
SHAPES = [(30, 20, "sym8", None), (6, 3, "sym8", None), (28, 100, "sym8", None), (13, 118, "sym8", 3500)]
plans = []
for cus in (256, 128):
    cases, keys = [], []
    for (n, T, lay, r2) in SHAPES:
        rows, cols, ld2, ld1 = shape(n, T, lay)
        for G in GS:
            cases.append(f"{r2 or rows} {cols} {ld2} {T} {n} {ld1} {G} {int(G > 1)} {int(T * T >= 1024)}")
            keys.append(dict(n=n, T=T, layout=lay, rows2=r2 or rows, count=G, cus=cus))
    out = subprocess.run([RECORDER, str(cus), "golden"], input="\n".join(cases) + "\n", capture_output=True, text=True, check=True).stdout
    blocks = out.split("CASE ")[1:]
    assert len(blocks) == len(keys)
    for k, b in zip(keys, blocks):
        lines = b.split("\n")[1:]
        assert not any(l.startswith(("ERROR", "NOTE", "K5 FAILED", "K8 FAILED")) for l in lines), b
        k["text"] = "\n".join(l for l in lines if l) + "\n"
        plans.append(k)
lib = C.CDLL(os.path.join(TREE, "evcont_amd", "libevcont_hip.so"))
for name, (res, args) in _lib.SIGNATURES.items():
    getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
ws = []
grid = [(n, T, lay) for lay in LAYOUT for (n, T) in [(1, 1), (4, 8), (6, 3), (10, 33), (13, 43), (14, 23), (20, 40), (28, 100), (30, 20), (33, 3), (40, 2), (64, 5)]]
grid += [(96, 1, "sym8"), (65, 2, "pack2"), (8, 160, "sym8"), (2, 130, "sym8"), (5, 512, "sym8")]
for (n, T, lay) in grid:
    rows, cols, ld2, ld1 = shape(n, T, lay)
    natm, count, npairs = 1 + n % 7, 1 + (n * T) % 37, 1 + T % 5
    t = TrdmSet(n=n, ntrain=T, layout=LAYOUT[lay], rows2=rows, row_offset=0, rows2_total=rows, cols2=cols, ld2=ld2, ld1=ld1, two_rdm=256, one_rdm=256, s_train=256)
    e = dict(n=n, T=T, layout=lay, natm=natm, count=count, npairs=npairs,
             workspace_bytes=lib.evc_workspace_bytes(C.byref(t), natm),
             workspace_bytes_batch=lib.evc_workspace_bytes_batch(C.byref(t), natm, count),
             workspace_bytes_roots_batch=lib.evc_workspace_bytes_roots_batch(C.byref(t), natm, count, npairs),
             gemv_rows_ws_bytes=lib.evc_gemv_rows_ws_bytes(rows, cols))
    assert e["workspace_bytes"] > 0, (n, T, lay, lib.evc_last_error())
    ws.append(e)
json.dump(dict(plans=plans, workspace=ws), open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "trdm_plan.json"), "w"), indent=0, separators=(",", ":"))
print(len(plans), len(ws))
