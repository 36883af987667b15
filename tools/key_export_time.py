#!/usr/bin/env python3
"""Wall time of zkr_key_export_websnark for the reference's tx circuit, BatchProcessTx(2, 6) at domain 2^17, and
for a synthetic 2^20 key: each key exported in ONE call, after one export of a 2^7 key that takes the loading of the kernels out
of the figures.  Per key: the total, its split as the call itself keeps it (zkr_key_export_last_times: kernels, copies through
the pinned buffer with the host copy to the output, the host writer of the header and pols sections; the rest of the total is
the allocation of the buffers and of the output), and the extra device memory at the peak -- the staging buffer the call reports
and the drop of the device's free memory as a second thread sees it while the call runs.  Also the registers and scratch of the
export kernels (tools/kernel_resources.py).  Writes the table to --out.
   python tools/key_export_time.py [--out profiles/key_export.md] [--log-m 20]"""
import argparse, os, subprocess, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import torch
import zkr_hip
from zkr_hip import rollup

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_export.md"))
ap.add_argument("--log-m", type=int, default=20)
a = ap.parse_args()
TOXIC = [0x1D0C5EED0123456789ABCDEF02468ACE13579BDF, 0x2468ACE013579BDF02468ACE13579BDF, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0, 0x5EED5EED5EED, 0x0CAFEBABEDEADBEEF0123456789ABCDEF]


def measure(name, key):
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    low, stop = [free0], threading.Event()

    def watch():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
            time.sleep(0.002)
    th = threading.Thread(target=watch)
    th.start()
    t0 = time.perf_counter()
    pkb = key.to_websnark()
    total = (time.perf_counter() - t0) * 1e3
    stop.set()
    th.join()
    t = key.export_times()
    info = key.info()
    back = torch.cuda.mem_get_info(0)[0]
    return dict(name=name, m=info["domainSize"], n=info["nVars"], nnz=info["nnzA"] + info["nnzB"], bytes=len(pkb), total=total, kernels=t["kernels_ms"], copies=t["copies_ms"],
                host=t["host_ms"], inside=t["total_ms"], staging=t["device_bytes"], seen=free0 - low[0], left=free0 - back)


warm, _, _ = zkr_hip.ProvingKey.synth(7, 7, want_aux=False)
warm.to_websnark()
warm.close()
rows = []
key, _ = zkr_hip.ProvingKey.setup_r1cs(rollup.RollupCircuit(2, 6).r1cs(), toxic=TOXIC)
rows.append(measure("tx circuit, BatchProcessTx(2, 6)", key))
key.close()
key, _, _ = zkr_hip.ProvingKey.synth(a.log_m, 73, want_aux=False)
rows.append(measure("synthetic 2^%d" % a.log_m, key))
key.close()

res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "zkr_key_export", "--all-kernels"], capture_output=True, text=True).stdout
lines = ["# zkr_key_export_websnark: one call per key", "",
         "`python tools/key_export_time.py` on one MI355X, %s.  One export of a 2^7 key first; then each key below in a single call," % zkr_hip.version(),
         "default piece of 2^20 points.  Milliseconds; MB = 10^6 bytes.", "",
         "| key | domain | nVars | terms A + B | output MB | total | kernels | copies | host writer | rest (allocations) | staging MB | free-memory drop seen MB | left behind |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
for r in rows:
    lines.append("| %s | 2^%d | %d | %d | %.1f | %.1f | %.2f | %.1f | %.1f | %.1f | %.1f | %.1f | %d B |" % (
        r["name"], r["m"].bit_length() - 1, r["n"], r["nnz"], r["bytes"] / 1e6, r["total"], r["kernels"], r["copies"], r["host"],
        r["total"] - r["kernels"] - r["copies"] - r["host"], r["staging"] / 1e6, r["seen"] / 1e6, r["left"]))
lines += ["", "Copies: device to pinned buffer on the call's stream, then pinned buffer to the output (the CSR arrays and every piece of",
          "every point section); host writer: the counting pass that turns the rows into per-signal lists.", "", "```", res.rstrip(), "```", ""]
open(a.out, "w").write("\n".join(lines))
print("\n".join(lines))
