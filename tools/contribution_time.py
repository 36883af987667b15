"""Times of a delta contribution (zkr_key_contribute) and of its verification (zkr_key_contribution_verify) beside the setup of
the same size, and the Fq-product count of the scaling kernel's schedule: host clock around each call (every one ends in a
device synchronise), median of REPS after one warm-up, all in one process so that the figures come from one box.
  python tools/contribution_time.py            the tx circuit (2^17, zkr_setup_r1cs) and a synthetic key at 2^20 (zkr_synth_key)
  python tools/contribution_time.py once 20    ONE contribution of a 2^20 key and nothing else: the run to put under
                                               `rocprofv3 --kernel-trace --stats -- python tools/contribution_time.py once 20`
                                               for the scaling kernel's own time (group_scale_uniform_kernel, two launches: C and H)
-> one JSON line per size.  fq_products: what the kernel's schedule multiplies for THIS d (csrc/kernels_group.hpp,
group_scale_uniform_kernel): per point `top` doublings of 9 products and one addition of 11 per non-zero NAF digit below the leading
one, 2 + 9 for the radix changes and the affine form, npt / 2 for the prefix products, and 1 / npt of an inversion."""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "simple-zk-rollups_amd", "python"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import zkr_hip

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
D = 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE
REPS = 5
DBL_PRODUCTS, ADD_PRODUCTS = 9, 11   # dbl_xyzz29: 4 squares + 3 products + the two-product Y form; add_mixed29: 2 + 7 + 2


def naf(e):
    out = []
    while e:
        z = 0
        if e & 1:
            z = 2 - (e & 3)
            e -= z
        out.append(z)
        e >>= 1
    return out


def products_per_point(d, n_points):
    digits = naf(pow(d, -1, R))
    top, adds = len(digits) - 1, sum(1 for z in digits[:-1] if z)
    npt = min(8, max(1, n_points // (1024 * 64 * 4)))          # group_scale_grid's points per thread
    inversion = 253 + bin(Q - 2).count("1")
    return top * DBL_PRODUCTS + adds * ADD_PRODUCTS + 2 + 9 + npt / 2 + inversion / npt, top, adds, npt


def median_ms(fn, reps=REPS):
    fn()                                                        # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return round(sorted(ts)[len(ts) // 2], 2)


def make_key(log_m):
    if log_m == 17:
        from zkr_hip import rollup as n
        r1cs = n.RollupCircuit(2, 6).r1cs()
        return lambda: zkr_hip.ProvingKey.setup_r1cs(r1cs)[0], "zkr_setup_r1cs"
    return lambda: zkr_hip.ProvingKey.synth(log_m, want_aux=False)[0], "zkr_synth_key"


def measure(log_m):
    make, how = make_key(log_m)
    key = make()
    info = key.info()
    n_scaled = info["ptsC"] + info["ptsH"]
    row = {"log_m": log_m, "setup_call": how, "points_scaled": n_scaled, "arena_MB": round(key.arena()[1] / 1e6, 1)}
    row["setup_ms"] = median_ms(lambda: make().close())
    k2, rec = key.contribute(D)
    assert key.contribution_verify(k2, rec) == (True, 0, 0)
    row["contribute_ms"] = median_ms(lambda: key.contribute(D)[0].close())
    row["contribution_verify_ms"] = median_ms(lambda: key.contribution_verify(k2, rec))
    per_c, top, adds, npt_c = products_per_point(D, info["ptsC"])
    per_h, _, _, npt_h = products_per_point(D, info["ptsH"])
    row["schedule"] = {"doublings": top, "additions": adds, "points_per_thread": [npt_c, npt_h]}
    row["fq_products"] = round(per_c * info["ptsC"] + per_h * info["ptsH"])
    row["fq_mul_G_per_s"] = round(zkr_hip.bench_fq_mul(), 1)
    k2.close()
    key.close()
    return row


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "once":
        key = make_key(int(sys.argv[2]))[0]()
        key.contribute(D)[0].close()
        key.close()
    else:
        for log_m in [int(a) for a in sys.argv[1:]] or [17, 20]:
            print(json.dumps(measure(log_m)), flush=True)
