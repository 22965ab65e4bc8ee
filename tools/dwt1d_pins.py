"""Maintenance of the pin tables of tests/test_gpu_dwt1d_routes.py after a deliberate dispatch change.

    python tools/dwt1d_pins.py record OUT.json [case id prefix ...]     on an MI355X: runs every case with the comparison against
                                                                        PINS off (the oracle comparisons stay on) and keeps the traces
    python tools/dwt1d_pins.py fill IN.json                             rewrites the PINS block from such a record

Read the diff of the test file afterwards: a route that changed without intent is a finding, not something to fill in.  REACHABLE
(the instances the dispatch can reach) is written by hand from the launchers and is never touched here: the closing test of the
module compares the regenerated PINS with it."""
import json
import os
import re
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def record(out, only):
    import wx_oracle
    wx_oracle.build()
    import waveletsext_jl_amd as wx
    import test_gpu_dwt1d_routes as T
    T.RECORD = {}
    fails, times = {}, {}
    jobs = [(c.id, lambda c=c: T.run_case(wx, wx_oracle, c)) for c in T.CASES_A]
    jobs += [(w.case.id, lambda w=w: T.run_wrap(wx, wx_oracle, w)) for w in T.WRAPS]
    for cid, job in jobs:
        if only and not any(cid.startswith(o) for o in only):
            continue
        t0 = time.time()
        try:
            job()
        except AssertionError as e:                       # a comparison failed: the kernels ran, go on
            fails[cid] = str(e)[:600]
            print("FAIL", cid, fails[cid], flush=True)
        except Exception:                                 # anything else (a HIP error): nothing more on this GPU
            fails[cid] = traceback.format_exc()[-1500:]
            print("ERROR, stopping at", cid, fails[cid], flush=True)
            break
        finally:
            wx.set_force_generic(0)
            times[cid] = time.time() - t0
            with open(out, "w") as f:
                json.dump({"record": T.RECORD, "fails": fails, "times": times}, f)
    print(len(times), "cases,", len(fails), "failures; slowest:", sorted(times.items(), key=lambda kv: -kv[1])[:5])
    return 1 if fails else 0


def _rows(v):
    if v is None:
        return "None"
    return "[" + ", ".join("(" + ", ".join(repr(x) for x in r) + ("," if len(r) == 1 else "") + ")" for r in v) + "]"


def fill(src):
    import test_gpu_dwt1d_routes as T
    with open(src) as f:
        d = json.load(f)
    R = d["record"]
    cases = {c.id: c for c in T.CASES_A}
    cases.update({w.case.id: w.case for w in T.WRAPS})
    lines = []
    for cid in cases:                                     # (the repeats under another dispatch mode, "case@mode", are checked, not pinned)
        f, i = R[cid]
        lines.append('    "%s": (%s,\n        %s),' % (cid, _rows(f), _rows(i)))
    p = os.path.join(ROOT, "tests", "test_gpu_dwt1d_routes.py")
    with open(p) as f:
        s = f.read()
    s = re.sub(r"# >>> PINS\n.*?# <<< PINS\n", lambda m: "# >>> PINS\nPINS = {\n" + "\n".join(lines) + "\n}\n# <<< PINS\n", s, flags=re.S)
    with open(p, "w") as f:
        f.write(s)
    print(len(lines), "cases; failures in the record:", d["fails"])
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "record":
        sys.exit(record(sys.argv[2], sys.argv[3:]))
    if len(sys.argv) == 3 and sys.argv[1] == "fill":
        sys.exit(fill(sys.argv[2]))
    sys.exit(__doc__)
