"""Time of one sharded proof (zkr_prove_sharded_device) with H in evaluation form against the coefficient form, the shards side by
side on ONE GPU: the same whole key cut twice, with and without side tables (ProvingKey.shard(side_tables=...)), the two shard sets
alternated in one process, `rounds` rounds of `n` proofs each.  Also the host times of the split calcH's phases
(zkr_prove_sharded_split_stats), mean over the shards, of the last proof of each form.  One JSON line per size.

  python tools/shard_eval_time.py [log_m:parts ...]      (default 16:2 20:8)

Shards on one device share its streams, so the numbers say what the forms cost in launches and butterflies; the traffic over the
links between GPUs that the evaluation form saves cannot be seen here (profiles/eval_h_sharded.md)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))


def measure(log_m, parts, rounds=3):
    import torch
    import zkr_hip
    key, wb, _ = zkr_hip.ProvingKey.synth(log_m, 73, 0x5A4B0001, 0x5A4B00FF, want_aux=False)
    assert key.h_form()["form"] == "evaluation"
    sets = {"evaluation": [key.shard(i, parts, side_tables=True) for i in range(parts)],
            "coefficients": [key.shard(i, parts) for i in range(parts)]}
    dw = torch.frombuffer(bytearray(wb), dtype=torch.uint8).cuda(0)
    torch.cuda.synchronize()
    ptrs = [dw.data_ptr()] * parts
    n = 10 if log_m >= 20 else 30
    proofs = {}
    for form, shards in sets.items():  # warm, and both forms give the same bytes
        for _ in range(2):
            proofs[form] = zkr_hip.prove_sharded_device(shards, ptrs, 31, 32)
        assert zkr_hip.sharded_last_h_form()["form"] == form
    assert proofs["evaluation"] == proofs["coefficients"] == key.prove(wb, 31, 32)
    out = {"log_m": log_m, "parts": parts, "proofs_per_round": n, "calc_h": zkr_hip.sharded_last_form()["form"], "ms_per_proof": {f: [] for f in sets}, "phase_ms": {}}
    for _ in range(rounds):
        for form, shards in sets.items():
            t0 = time.perf_counter()
            for _ in range(n):
                zkr_hip.prove_sharded_device(shards, ptrs, 31, 32)
            out["ms_per_proof"][form].append(round((time.perf_counter() - t0) * 1e3 / n, 3))
            stats = zkr_hip.sharded_split_stats()
            if stats is not None:
                out["phase_ms"][form] = [round(sum(row[p] for row in stats) / parts, 3) for p in range(5)]
    for shards in sets.values():
        for sh in shards:
            sh.close()
    key.close()
    return out


if __name__ == "__main__":
    cases = [tuple(int(x) for x in a.split(":")) for a in sys.argv[1:]] or [(16, 2), (20, 8)]
    for log_m, parts in cases:
        print(json.dumps(measure(log_m, parts)), flush=True)
