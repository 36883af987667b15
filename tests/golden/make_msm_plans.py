"""Record what msm_plan returns into tests/golden/msm_plans.json: (n_scalars, n_points, c_fixed) -> the ten plan fields
c, K, glog, nbw, nb, big_thresh, nR, nbl, J, S.  tests/test_proof_layout_cpu.py holds every later msm_plan against this file, so it
is run on the commit whose values are to be kept (build first):  python tests/golden/make_msm_plans.py

The plan is read through the host shim (zkt_msm_plan) where the shim has it; a commit from before that keeps msm_plan inside
libzkr_hip.so only, and the script calls the C++ symbol there (a plain struct of ten 32-bit words returned by value; loading the
library needs no GPU)."""
import ctypes
import json
import os

os.environ.pop("ZKR_MSM_C", None)  # the window knob would override every plan
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "simple-zk-rollups_amd", "csrc")
FIELDS = ["c", "K", "glog", "nbw", "nb", "big_thresh", "nR", "nbl", "J", "S"]


def cases():
    free = [(1, 1), (5, 1), (100, 73), (1 << 7, 100), (1 << 10, 700), (1 << 12, 1 << 12), (1 << 12, 1), ((1 << 13) + 1, 5000),
            (1 << 17, 1 << 17), (1 << 17, 87000), (1 << 20, 1 << 20), (1 << 20, 1013000), (1 << 20, 1), (1 << 22, 1 << 22),
            (1 << 24, 1 << 24), (1 << 24, 11000000)]
    out = [(ns, npt, 0) for ns, npt in free]
    out += [(1 << 20, 1013000, c) for c in range(2, 23)]           # every window the library accepts, on a table of the flagship size
    out += [(1 << 12, 3000, c) for c in (2, 8, 13, 22)] + [(1 << 24, 1 << 24, 22), (64, 1, 2)]
    return out


def planner():
    shim = ctypes.CDLL(os.path.join(CSRC, "libzkr_hostarith.so"))
    if hasattr(shim, "zkt_msm_plan"):
        shim.zkt_msm_plan.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
        shim.zkt_msm_plan.restype = None

        def plan(ns, npt, c):
            out = (ctypes.c_uint32 * 10)()
            shim.zkt_msm_plan(ns, npt, c, out)
            return list(out)
        return plan, "host shim"

    class Plan(ctypes.Structure):
        _fields_ = [(f, ctypes.c_uint32) for f in FIELDS]
    fn = getattr(ctypes.CDLL(os.path.join(CSRC, "libzkr_hip.so")), "_ZN3zkr8msm_planEmmi")  # zkr::msm_plan(unsigned long, unsigned long, int)
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    fn.restype = Plan
    return (lambda ns, npt, c: [getattr(fn(ns, npt, c), f) for f in FIELDS]), "libzkr_hip.so"


if __name__ == "__main__":
    plan, source = planner()
    rows = [{"n_scalars": ns, "n_points": npt, "c_fixed": c, "plan": plan(ns, npt, c)} for ns, npt, c in cases()]
    with open(os.path.join(HERE, "msm_plans.json"), "w") as f:   # one plan per line
        f.write('{"fields": %s,\n "plans": [\n  %s\n ]}\n' % (json.dumps(FIELDS), ",\n  ".join(json.dumps(r) for r in rows)))
    print(len(rows), "plans from the", source)
