"""Time of the witness check (zkr_r1cs_check_device) beside what it can stand in for and what it guards, in one process: the tx
circuit BatchProcessTx(2, 6) at 2^17 -- a lone witness and a fused batch of zkr_key_fuse witnesses already in HBM -- and
BatchProcessTx(18, 6) at 2^20; next to each, zkr_verify on a proof of that circuit and the proof itself.  One warm-up, median of
ten, host clock around calls that end in a synchronise.  Terms per second count every term of A, B and C once per witness; bytes
per second take 68 B per term (36 B of term, a 32 B gather).
python tools/r1cs_check_time.py [out.md]   -> one JSON line per case, and the table as markdown when a path is given"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "simple-zk-rollups_amd", "python"))
import torch, zkr_hip
from zkr_hip import rollup

REPS = 10


def median_ms(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    ts.sort()
    return round(ts[len(ts) // 2], 3)


def flats_for(circ, n):
    privs = [0x5A4B1000 + 7919 * i for i in range(8)]
    st = rollup.RollupState(circ.depth)
    for i, pv in enumerate(privs):
        st.deposit(i, rollup.gen_public_key(pv), 10 ** 24, 0)
    out = []
    for b in range(n):
        txs = [st.transfer((circ.batch * b + j) % 8, (circ.batch * b + j + 3) % 8, 10 ** 15 * (j + 1) + b, 10 ** 12, privs[(circ.batch * b + j) % 8]) for j in range(circ.batch)]
        out.append(circ.flatten_inputs(st.batch_inputs(txs)))
    return out


rows = []
for batch, depth in ((2, 6), (18, 6)):
    circ = rollup.RollupCircuit(batch, depth)
    r1cs = circ.r1cs()
    key, vk = zkr_hip.ProvingKey.setup_r1cs(r1cs)
    cs = zkr_hip.ConstraintSystem.load(r1cs)
    assert cs.matches_key(key)
    info = cs.info()
    terms = info["nnzA"] + info["nnzB"] + info["nnzC"]
    fuse = key.fuse()
    dev = circ.calculate_witness_batch_device(flats_for(circ, fuse))
    torch.cuda.synchronize()
    ptrs = [dev[i].data_ptr() for i in range(fuse)]
    assert cs.check_device(ptrs)[0] is True
    proofs = key.prove_batch_device(ptrs)
    pub = circ.public_signals(bytes(dev[0].cpu().numpy().tobytes()))
    assert zkr_hip.verify(vk, proofs[0], pub)
    row = {"circuit": "BatchProcessTx(%d, %d)" % (batch, depth), "domain_log2": key.info()["domainSize"].bit_length() - 1, "constraints": info["nConstraints"],
           "terms": terms, "fuse": fuse,
           "check_1_ms": median_ms(lambda: cs.check_device(ptrs[:1])),
           "verify_ms": median_ms(lambda: zkr_hip.verify(vk, proofs[0], pub)),
           "prove_1_ms": median_ms(lambda: key.prove_device(ptrs[0])),
           "matches_key_ms": median_ms(lambda: cs.matches_key(key))}
    if fuse > 1:
        row["check_fused_ms"] = median_ms(lambda: cs.check_device(ptrs))
        row["prove_fused_ms"] = median_ms(lambda: key.prove_batch_device(ptrs))
    n, ms = (fuse, row["check_fused_ms"]) if fuse > 1 else (1, row["check_1_ms"])
    row["Gterms_per_s"] = round(n * terms / ms / 1e6, 2)
    row["GB_per_s"] = round(68 * n * terms / ms / 1e6, 1)
    rows.append(row)
    print(json.dumps(row), flush=True)
    cs.close()
    key.close()

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("| circuit | domain | constraints | terms | check, 1 witness (ms) | check, fused batch (ms) | per witness (ms) | zkr_verify (ms) | proof, lone (ms) | proof, fused, per proof (ms) | matches_key (ms) | G terms/s | GB/s at 68 B/term |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            fused = "%s (%d)" % (r["check_fused_ms"], r["fuse"]) if "check_fused_ms" in r else "-"
            per = round(r["check_fused_ms"] / r["fuse"], 4) if "check_fused_ms" in r else r["check_1_ms"]
            pf = round(r["prove_fused_ms"] / r["fuse"], 3) if "prove_fused_ms" in r else "-"
            f.write("| %s | 2^%d | %d | %d | %s | %s | %s | %s | %s | %s | %s | %s | %s |\n" % (r["circuit"], r["domain_log2"], r["constraints"], r["terms"], r["check_1_ms"], fused, per,
                                                                                              r["verify_ms"], r["prove_1_ms"], pf, r["matches_key_ms"], r["Gterms_per_s"], r["GB_per_s"]))
