"""Time of zkr_key_check at levels 0 (structure: the index arrays) and 1 (structure + values: the whole arena) on synthetic keys:
host clock around the call, which returns after its own stream has finished; one warm-up call per level first.
python tools/key_check_time.py [log_m ...]   (default 20; 22 as well when given) -> one JSON line per size"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "simple-zk-rollups_amd", "python"))
import zkr_hip

REPS = 10
for log_m in [int(a) for a in sys.argv[1:]] or [20]:
    key, _, _ = zkr_hip.ProvingKey.synth(log_m, want_aux=False)
    arena_mb = key.arena()[1] / 1e6
    row = {"log_m": log_m, "arena_MB": round(arena_mb, 1)}
    for level in (0, 1):
        assert key.check(level)["bad"] == 0        # warm-up (and the key is clean)
        ts = []
        for _ in range(REPS):
            t = time.perf_counter()
            key.check(level)
            ts.append(1e3 * (time.perf_counter() - t))
        ts.sort()
        row["level%d_ms" % level] = {"min": round(ts[0], 3), "median": round(ts[len(ts) // 2], 3), "max": round(ts[-1], 3)}
    row["level1_GBps"] = round(arena_mb / 1e3 / (row["level1_ms"]["median"] / 1e3), 1)
    key.close()
    print(json.dumps(row), flush=True)
