"""The evaluation-form side tables derived from a key's own points (zkr_key_eval_tables), measured on the keys a deployment proves
with: a transcript key (zkr_setup_r1cs_ptau) after a delta contribution (zkr_key_contribute).  One MI355X, ONE process.
  python tools/eval_tables_time.py [out.md] [log_m ...]      default: profiles/eval_tables_from_points.md, sizes 17 and 20
Per size (2^17: the tx circuit BatchProcessTx(2, 6) with a transcript of power 17; 2^20: BatchProcessTx(18, 6), power 20):
  derivation   zkr_key_eval_tables in ms, host clock (the call ends in a device synchronise), median of five after one warm-up,
               with zkr_setup_r1cs_ptau of the same circuit beside it for scale; free device memory before and after the build
At the largest size also, on the same contributed transcript key:
  proof rate   two proofs in flight (prove_batch_device, depth 2), the witness resident in HBM; without tables / with tables /
               dropped / rebuilt, three rounds.  The yardstick is the key's OWN coefficient-form rate in the same process; reported
               as profiles/eval_h_parent_vs_tree.md reports its comparison: slowest evaluation-form run against fastest
               coefficient-form run, the means, and each form's spread
  bytes        the proofs of the two forms are identical"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import torch, zkr_hip
from zkr_hip import rollup

SECRETS = (0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F7081, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978, 0x123456789ABCDEF0FEDCBA9876543210123456789ABCDEF)
D = 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE
CIRCUITS = {17: (2, 6), 20: (18, 6)}   # BatchProcessTx(batch, depth)
REPS, ROUNDS, PROOFS, WARM = 5, 3, 60, 6


def median_ms(fn, reps=REPS):
    fn()                                                        # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return round(sorted(ts)[len(ts) // 2], 2)


def free_gb():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0] / 1e9


def witness(circ, batch):
    privs = [0x5A4B1000 + 7919 * i for i in range(8)]
    st = rollup.RollupState(6)
    for i, pv in enumerate(privs):
        st.deposit(i, rollup.gen_public_key(pv), 10 ** 20, 0)
    txs = [st.transfer(j % 8, (j + 3) % 8, 10 ** 17, 10 ** 15, privs[j % 8]) for j in range(batch)]
    return circ.calculate_witness(st.batch_inputs(txs))


def rate(key, d_w, n):
    ptrs = [d_w.data_ptr()] * n
    key.prove_batch_device(ptrs[:WARM], depth=2)
    torch.cuda.synchronize()
    t = time.perf_counter()
    key.prove_batch_device(ptrs, depth=2)
    return n / (time.perf_counter() - t)


def measure(log_m, with_rate):
    circ = rollup.RollupCircuit(*CIRCUITS[log_m])
    r1cs = circ.r1cs()
    ptau, _ = zkr_hip.ptau_contribute(zkr_hip.ptau_new(log_m), SECRETS)
    row = {"log_m": log_m}
    row["setup_r1cs_ptau_ms"] = median_ms(lambda: zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, ptau)[0].close())
    k0, _ = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, ptau)
    key, _ = k0.contribute(D)
    k0.close()
    del ptau
    row["key"] = key.info()
    key.base_arena()                                            # the compact arena the derivation reads is cached on the key: not the tables' memory
    before = free_gb()
    assert key.eval_tables(r1cs), zkr_hip.lib().zkr_last_error().decode()
    row["tables_GB"] = round(before - free_gb(), 3)
    key.drop_eval_tables()
    row["after_drop_GB"] = round(before - free_gb(), 3) or 0.0
    row["eval_tables_ms"] = median_ms(lambda: key.eval_tables(r1cs))
    key.drop_eval_tables()
    if with_rate:
        wb = witness(circ, CIRCUITS[log_m][0])
        d_w = torch.frombuffer(bytearray(wb), dtype=torch.uint8).cuda()
        r, s = 0x1234567890ABCDEF, 0x0FEDCBA987654321
        runs = {"without": [], "with": [], "dropped": [], "rebuilt": []}
        proofs = {}
        for _ in range(ROUNDS):
            for phase in ("without", "with", "dropped", "rebuilt"):
                if phase in ("with", "rebuilt"):
                    assert key.eval_tables(r1cs)
                else:
                    key.drop_eval_tables()
                assert key.h_form()["form"] == ("evaluation" if phase in ("with", "rebuilt") else "coefficients")
                runs[phase].append(round(rate(key, d_w, PROOFS), 2))
                proofs.setdefault(phase, key.prove(wb, r, s))
        coef, ev = runs["without"] + runs["dropped"], runs["with"] + runs["rebuilt"]
        spread = lambda v: round(100 * (max(v) / min(v) - 1), 2)
        row["proofs_per_s"] = runs
        row["coefficient_form"] = {"min": min(coef), "max": max(coef), "mean": round(sum(coef) / len(coef), 2), "spread_pct": spread(coef)}
        row["evaluation_form"] = {"min": min(ev), "max": max(ev), "mean": round(sum(ev) / len(ev), 2), "spread_pct": spread(ev)}
        row["slowest_eval_vs_fastest_coef_pct"] = round(100 * (min(ev) / max(coef) - 1), 2)
        row["means_pct"] = round(100 * (sum(ev) / len(ev) / (sum(coef) / len(coef)) - 1), 2)
        row["retries"] = key.h_form()["retries"]
        row["proofs_identical"] = len(set(proofs.values())) == 1
    key.close()
    return row


def render(rows):
    out = ["# Evaluation-form side tables derived from a key's own points: times, memory, proof rate (one MI355X, one process)", "",
           "`python tools/eval_tables_time.py`: a transcript key (`zkr_setup_r1cs_ptau`) after one `zkr_key_contribute`, the kind of key a",
           "deployment proves with.  2^17: the tx circuit `BatchProcessTx(2, 6)`, transcript of power 17; 2^20: `BatchProcessTx(18, 6)`, power 20.",
           "Times: host clock around the call, median of five after one warm-up.  Memory: free device memory before and after the build",
           "(the compact arena the derivation reads was cached on the key before).", "",
           "| domain | `zkr_key_eval_tables` ms | `zkr_setup_r1cs_ptau` ms | tables GB | still held after the drop GB |", "|---|---|---|---|---|"]
    for r in rows:
        out.append("| 2^%d | %.2f | %.2f | %.3f | %.3f |" % (r["log_m"], r["eval_tables_ms"], r["setup_r1cs_ptau_ms"], r["tables_GB"], r["after_drop_GB"]))
    for r in rows:
        if "proofs_per_s" not in r:
            continue
        c, e = r["coefficient_form"], r["evaluation_form"]
        out += ["", "## Proof rate at 2^%d, the same key in both forms (two proofs in flight, %d proofs per run, proofs/s)" % (r["log_m"], PROOFS), "",
                "| round | without tables | with tables | dropped | rebuilt |", "|---|---|---|---|---|"]
        for i in range(ROUNDS):
            out.append("| %d | %s |" % (i + 1, " | ".join("%.2f" % r["proofs_per_s"][p][i] for p in ("without", "with", "dropped", "rebuilt"))))
        out += ["", "Coefficient form %.2f .. %.2f (spread %.2f %%), evaluation form %.2f .. %.2f (%.2f %%).  The slowest evaluation-form run is %+.2f %%"
                % (c["min"], c["max"], c["spread_pct"], e["min"], e["max"], e["spread_pct"], r["slowest_eval_vs_fastest_coef_pct"]),
                "against the fastest coefficient-form run; means %.2f and %.2f, %+.2f %%.  Retries: %d.  Proofs of the two forms identical: %s."
                % (c["mean"], e["mean"], r["means_pct"], r["retries"], "yes" if r["proofs_identical"] else "NO")]
        out.append("The parent comparison of `profiles/eval_h_parent_vs_tree.md` recorded a run-to-run spread of 0.7 %% and +2.6 %% for the same statistic: this difference is %s that spread."
                   % ("outside" if abs(r["slowest_eval_vs_fastest_coef_pct"]) > 0.7 else "INSIDE"))
    out += ["", "```"] + [json.dumps(r) for r in rows] + ["```", ""]
    return "\n".join(out)


if __name__ == "__main__":
    args = sys.argv[1:]
    path = args.pop(0) if args and not args[0].isdigit() else os.path.join(ROOT, "profiles", "eval_tables_from_points.md")
    sizes = [int(a) for a in args] or [17, 20]
    rows = []
    for log_m in sizes:
        rows.append(measure(log_m, log_m == max(sizes)))
        print(json.dumps(rows[-1]), flush=True)
    with open(path, "w") as f:
        f.write(render(rows))
