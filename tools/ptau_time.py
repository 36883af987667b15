"""Times of the powers-of-tau calls -- a contribution (zkr_ptau_contribute), the verification of a transcript (zkr_ptau_verify) and
the setup of a key from it (zkr_setup_r1cs_ptau) -- beside the one-party setup of the same circuit (zkr_setup_r1cs) IN THE SAME
PROCESS: host clock around each call (every one ends in a device synchronise), median of REPS after one warm-up.
  python tools/ptau_time.py            the tx circuit BatchProcessTx(2, 6) (2^17) and BatchProcessTx(18, 6) (2^20)
  python tools/ptau_time.py 17         one size
  python tools/ptau_time.py once 17    ONE contribution and ONE setup from the transcript and nothing else: the run to put under
                                       `rocprofv3 --kernel-trace --stats -- python tools/ptau_time.py once 17` for the kernels' own times
-> one JSON line per size.  fq_products: the paper count of the two big kernels for that size -- a variable-base multiplication
by a lane's own scalar is 254 doublings of 9 products and (on average) 127 additions of 11 that the whole wavefront executes in
practically every step, 254 x 20 = 5 080 per G1 point; a contribution multiplies 4 M G1 and M G2 points, the four inverse
transforms of a setup log2(m) - 1 stages of m / 2 multiplications each plus m for the factor 1 / m (G2: three Fq products per
Fq2 product)."""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "simple-zk-rollups_amd", "python"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import zkr_hip

SECRETS = (0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F7081, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978, 0x123456789ABCDEF0FEDCBA9876543210123456789ABCDEF)
REPS = 5
MUL_PRODUCTS, G2_FACTOR = 254 * (9 + 11), 3


def median_ms(fn, reps=REPS):
    fn()                                                        # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return round(sorted(ts)[len(ts) // 2], 2)


CIRCUITS = {17: (2, 6), 20: (18, 6)}   # BatchProcessTx(batch, depth): the reference's tx circuit, and the same template filled to 2^20


def circuit(log_m):
    from zkr_hip import rollup as n
    return n.RollupCircuit(*CIRCUITS[log_m]).r1cs()


def measure(log_m):
    r1cs = circuit(log_m)
    M = 1 << log_m
    start = zkr_hip.ptau_new(log_m)
    t, rec = zkr_hip.ptau_contribute(start, SECRETS)
    assert zkr_hip.ptau_verify(t, [rec]) == (True, 0, 0)
    row = {"log_m": log_m, "transcript_MB": round(len(t) / 1e6, 1)}
    row["ptau_contribute_ms"] = median_ms(lambda: zkr_hip.ptau_contribute(start, SECRETS))
    row["ptau_verify_ms"] = median_ms(lambda: zkr_hip.ptau_verify(t, [rec]))
    row["setup_r1cs_ptau_ms"] = median_ms(lambda: zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, t)[0].close())
    row["setup_r1cs_ms"] = median_ms(lambda: zkr_hip.ProvingKey.setup_r1cs(r1cs)[0].close())
    row["fq_products"] = {"contribute": MUL_PRODUCTS * (4 * M + G2_FACTOR * M),
                          "setup_transforms": MUL_PRODUCTS * (3 + G2_FACTOR) * ((log_m - 1) * M // 2 + M)}
    row["fq_mul_G_per_s"] = round(zkr_hip.bench_fq_mul(), 1)
    return row


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "once":
        log_m = int(sys.argv[2])
        t, _ = zkr_hip.ptau_contribute(zkr_hip.ptau_new(log_m), SECRETS)
        zkr_hip.ProvingKey.setup_r1cs_ptau(circuit(log_m), t)[0].close()
    else:
        for log_m in [int(a) for a in sys.argv[1:]] or [17, 20]:
            print(json.dumps(measure(log_m)), flush=True)
