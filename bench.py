#!/usr/bin/env python3
"""bench.py -- Groth16 proofs/sec of the MI355X prover on the synthetic rollup circuit.

Contract: python bench.py --gpus N --steps K --warmup W   (N>1: launched by torch.distributed.run,
one rank per GPU).  A step = one proof (QAP rows -> 6 NTTs -> 5 MSMs -> assembly) of the m = 2^20
rollup-shaped circuit with 73 public inputs (BASELINE.json configs[1]); witnesses are resident in
HBM when the timed region starts.  N>1: the key is generated on rank 0 and broadcast over RCCL, each
rank proves its own K witnesses (weak scaling, no data-path collective).  Prints ONE JSON line.

A plain run does only what the headline needs: set-up, W warm-up steps, K timed steps, the result line (metric, value,
unit, higher_is_better, dtype, ms_per_step = milliseconds of one timed step).  --full adds everything else the line has
carried: stage profile and roofline, sampled clock and power, the native check of every timed proof, the calling-pattern
boundary, the CPU baselines, the replication, sharding, other-size and other-circuit legs (the --no-* options trim it).
--dump-outputs DIR writes the proofs of the last timed step as DIR/pi_a.npy, pi_b.npy, pi_c.npy (dump_outputs); the
inputs are seeded, so two builds run with the same arguments can be compared output for output.

Other forms (same JSON shape):  --gpus N --inproc [--devices 0,0]   N devices from ONE process through zkr_key_replicate +
zkr_prove_batch_multi_device (no torch.distributed: the shape of the reference's Node host);  --shards P   (default 8; 0 skips) is the
intra-proof sharding leg (one proof cut into P shards, each timed alone: projected one-shard-per-GPU latency);
--log-m 22 / 24, --shape dense: the other BASELINE configs;  --no-pipeline: synchronous proofs.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
ROUND = 6                                  # the counter files bench.py quotes must be THIS round's (profiles/r6_*): older kernels' traffic is not carried over
PMC_FILE = "r%d_pmc_traffic.json" % ROUND  # HBM traffic per kernel (tools/profile_round6.sh part b)
CENSUS_FILE = "r%d_valu_census.json" % ROUND  # VALU wave-instructions per proof by SQ counters (profiles/summarize_census.py)
# Group additions in units of one Fq Montgomery multiplication of the hot path (csrc/field29.hpp: 9 x 29-bit limbs, 162
# 32x32 multiply-adds: 81 for the product, 81 for the reduction).  A square takes its off-diagonal products once (45 + 81),
# the Y coordinate of an addition is a difference of two products with ONE reduction (2 x 81 + 81), an Fq2 product is two
# such sums, an Fq2 square one such sum and one product, the Y coordinate over Fq2 two sums of four products (csrc/curve29.hpp):
MUL, SQR, SUM2, SUM4 = 162.0, 126.0, 243.0, 405.0
MADD_G1 = (6 * MUL + 2 * SQR + SUM2) / MUL                              # XYZZ += affine, 8M + 2S            ->  9.06
MADD_G2 = (6 * 2 * SUM2 + 2 * (SUM2 + MUL) + 2 * SUM4) / MUL            # the same over Fq2                  -> 28.0
ADD_G1 = (10 * MUL + 2 * SQR + SUM2) / MUL                              # XYZZ += XYZZ, 12M + 2S             -> 13.06
ADD_G2 = (10 * 2 * SUM2 + 2 * (SUM2 + MUL) + 2 * SUM4) / MUL            # the same over Fq2                  -> 40.0
MADS_PER_MUL = 162
CIRCUIT_SEED, TOXIC_SEED, N_PUBLIC = 0x5A4B0001, 0x5A4B00FF, 73


def effective_host_cores():
    """Hardware threads this process may really use: the smallest of the CPU count, the affinity mask and the cgroup CPU
    quota (the GPU boxes of the pool show 256 hardware threads but run the job under a 16-CPU quota: 128 or 256 OpenMP
    threads are then SLOWER than 16, profiles/r2_cpu_oracle_thread_scaling.txt)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
            break
        except Exception:
            continue
    return n


def cpu_baseline(sample_log_m, target_log_m, gpu_key=None):
    """The C oracle (oracle/zkr_oracle.c) on the host cores of this box, on a key of the same generator (websnark
    buffer rendered by the product, fed to the oracle's own parser): zo_prove on ONE thread and zo_prove_mt on ALL
    hardware threads (OpenMP), both MEASURED at m = 2^sample_log_m -- by default the benchmarked size itself, so
    nothing is extrapolated ("1 thread and all host threads at the real config sizes").  The two CPU
    proofs and, when the sizes agree, the GPU proof for the same blinding must be the same bytes."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import coracle
    import zkr_hip
    # BASELINE.md section 3 promises `-O3 -march=native`: the shipped library is the portable x86-64-v2 build (it has to run on
    # whatever CPU the box has), so a native one is compiled here, on this host, before the first call, and the faster of the two
    # on a small proof is the one timed (on the EPYC 9575F boxes gcc 11's -march=native came out 10 % SLOWER)
    build = coracle.use_fastest(*zkr_hip.synth_websnark(14, N_PUBLIC, CIRCUIT_SEED, TOXIC_SEED, device=0))   # native or portable, whichever is faster HERE
    pkb, wb = zkr_hip.synth_websnark(sample_log_m, N_PUBLIC, CIRCUIT_SEED, TOXIC_SEED, device=0)
    r, s = 12345, 67890
    t0 = time.time()
    p1, tm = coracle.prove(pkb, wb, r, s, want_timings=True)
    dt = time.time() - t0
    t0 = time.time()
    pm, tmm = coracle.prove_mt(pkb, wb, r, s, threads=effective_host_cores(), want_timings=True)
    dtm = time.time() - t0
    same = p1 == pm
    if gpu_key is not None and sample_log_m == target_log_m:
        same = same and gpu_key.prove(wb, r, s) == p1
    scale = 2.0 ** (target_log_m - sample_log_m)
    how = "measured at m=2^%d (the benchmarked size, no extrapolation)" % sample_log_m if scale == 1.0 else \
          "measured at m=2^%d, value = 1/(t * 2^%d) i.e. linearly scaled to m=2^%d" % (sample_log_m, target_log_m - sample_log_m, target_log_m)
    return {"value": 1.0 / (dt * scale), "unit": "proofs/s", "cores": 1, "kind": "port",
            # short: the driver's record keeps the first 120 characters of a string
            "sample": "C oracle zo_prove, 1 thread, one 2^%d proof %s: %.1f s (calcH %.1f + MSM %.1f); gcc -O3 -march=%s" % (
                sample_log_m, "MEASURED" if scale == 1.0 else "measured, scaled x2^%d" % (target_log_m - sample_log_m), dt, tm[0], tm[1],
                "native" if "march=native" in build else "x86-64-v2"),
            "sample_detail": how,
            "seconds_per_proof": dt * scale, "build": build,
            # the same figures as scalars: the driver's record keeps scalars and short strings only
            "all_threads_proofs_per_s": 1.0 / (dtm * scale), "all_threads_cores": int(tmm[3]), "all_threads_seconds_per_proof": dtm * scale,
            "all_threads": {"value": 1.0 / (dtm * scale), "unit": "proofs/s", "cores": int(tmm[3]), "kind": "port",
                            "sample": "oracle/zkr_oracle.c zo_prove_mt (OpenMP: five multiexps cut into point slices, parallel NTT butterflies), %d threads, "
                                      "same key and witness: %.2f s (calcH %.2f s, MSM %.2f s); %s" % (int(tmm[3]), dtm, tmm[0], tmm[1], how),
                            "seconds_per_proof": dtm * scale},
            "cpu_and_gpu_proofs_identical": bool(same)}


def cpu_baseline_js(sample_log_m, target_log_m):
    """oracle/cpu_ref_js.js: single-thread snarkjs-0.1.20-shaped genProof (one double-and-add scalar
    multiplication per signal and query, native BigInt) on a small key of the same generator, scaled linearly in
    m.  snarkjs itself is not installable here; this restates its algorithm and is pinned against
    the closed form in tests/test_oracle.py."""
    import shutil
    import subprocess
    import tempfile
    node = shutil.which("node")
    if node is None:
        return {"error": "node is not available on this box"}
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import groth16 as g
    import zkr_hip
    pkb, wb = zkr_hip.synth_websnark(sample_log_m, N_PUBLIC, CIRCUIT_SEED, TOXIC_SEED, device=0)
    jk = g.to_json_key(g.parse_proving_key(pkb))

    def js(x):
        if isinstance(x, bool) or x is None:
            return x
        if isinstance(x, int):
            return str(x)
        if isinstance(x, dict):
            return {str(k): js(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [js(v) for v in x]
        return x
    key = js(jk)
    for f in ("nVars", "nPublic", "domainSize"):
        key[f] = int(key[f])
    wit = [str(int.from_bytes(wb[32 * i:32 * i + 32], "little")) for i in range(len(wb) // 32)]
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump({"pk": key, "witness": wit, "r": "12345", "s": "67890"}, f)
        path = f.name
    try:
        out = subprocess.run([node, os.path.join(ROOT, "oracle", "cpu_ref_js.js"), path], capture_output=True, text=True, timeout=900)
    finally:
        os.unlink(path)
    if out.returncode != 0:
        return {"error": out.stderr[-300:]}
    sec = json.loads(out.stdout)["seconds"]
    scale = 2.0 ** (target_log_m - sample_log_m)
    return {"value": 1.0 / (sec["total"] * scale), "unit": "proofs/s", "cores": 1, "kind": "port",
            "sample": "oracle/cpu_ref_js.js (snarkjs-0.1.20-shaped genProof, node %s, native BigInt, 1 thread), m=2^%d key: %.1f s/proof "
                      "(calculateH %.1f s, per-signal scalar multiplications %.1f s); value = 1/(t * 2^%d)"
                      % (subprocess.run([node, "--version"], capture_output=True, text=True).stdout.strip(), sample_log_m, sec["total"],
                         sec["h"], sec["msm"], target_log_m - sample_log_m)}


def cpu_baseline_scalars(cb, gpu_proofs_per_s, js_sample_log_m):
    """The north star's ratios ("x snarkjs single-thread CPU", BASELINE.json) as SCALARS of `cpu_baseline`: the driver's record
    keeps scalars and short strings only, so the nested `snarkjs_style` object (the denominator of the >= 50x claim) is repeated
    flat, next to the ratios against the C oracle on one thread and on all host threads."""
    js_leg = cb.get("snarkjs_style") or {}
    v = js_leg.get("value")
    cb["snarkjs_style_proofs_per_s"] = v
    cb["snarkjs_style_sample_log_m"] = js_sample_log_m if v else None
    cb["snarkjs_style_seconds_per_proof"] = (1.0 / v) if v else None
    cb["speedup_vs_snarkjs_style"] = (gpu_proofs_per_s / v) if v else None
    cb["speedup_vs_c_1thread"] = (gpu_proofs_per_s / cb["value"]) if cb.get("value") else None
    cb["speedup_vs_c_all_threads"] = (gpu_proofs_per_s / cb["all_threads_proofs_per_s"]) if cb.get("all_threads_proofs_per_s") else None
    return cb


class GpuSampler:
    """Device clock (MHz) and board power (W) sampled from sysfs while the timed region runs (the sustained
    clock under this integer load must be a recorded number, not an inference).  Sources, first that works:
    hwmon freq1_input / power1_average|power1_input of the amdgpu device, pp_dpm_sclk's starred level, `rocm-smi`."""

    def __init__(self, index=0, period=0.05):
        import glob
        import threading
        self.period, self.samples, self._stop = period, [], threading.Event()
        self.dev = None
        try:  # the sysfs node of THIS HIP device (a node has eight GPUs, and more DRM cards than GPUs)
            import zkr_hip
            pci = zkr_hip.device_pci_bus_id(index).lower()
            cand = "/sys/bus/pci/devices/" + pci
            if os.path.isdir(cand):
                self.dev = cand
            self.pci = pci
        except Exception:
            self.pci = None
        if self.dev is None:
            cards = sorted(glob.glob("/sys/class/drm/card[0-9]*/device"))
            cards = [c for c in cards if glob.glob(os.path.join(c, "hwmon/hwmon*/freq1_input"))]
            self.dev = cards[index] if index < len(cards) else (cards[0] if cards else None)
        self.hw = (glob.glob(os.path.join(self.dev, "hwmon/hwmon*")) or [None])[0] if self.dev else None
        self.source = None
        self._thread = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return f.read()
        except Exception:
            return None

    def _one(self):
        mhz = watts = None
        if self.hw:
            v = self._read(os.path.join(self.hw, "freq1_input"))
            if v and v.strip().isdigit():
                mhz = int(v) / 1e6
            for name in ("power1_average", "power1_input"):
                v = self._read(os.path.join(self.hw, name))
                if v and v.strip().isdigit():
                    watts = int(v) / 1e6
                    break
        if mhz is None and self.dev:
            v = self._read(os.path.join(self.dev, "pp_dpm_sclk"))
            if v:
                for ln in v.splitlines():
                    if ln.strip().endswith("*"):
                        try:
                            mhz = float(ln.split(":")[1].lower().replace("mhz", "").replace("*", "").strip())
                        except Exception:
                            pass
        return mhz, watts

    def _run(self):
        while not self._stop.is_set():
            self.samples.append(self._one())
            self._stop.wait(self.period)

    def start(self):
        mhz, watts = self._one()
        self.source = "sysfs %s" % self.dev if (mhz is not None or watts is not None) else None
        if self.source:
            self._thread.start()
        return self

    def stop(self):
        self._stop.set()
        if self._thread.is_alive():
            self._thread.join(1.0)
        out = {"source": self.source, "pci_bus_id": getattr(self, "pci", None), "samples": len(self.samples)}
        mh = [m for m, _ in self.samples if m]
        pw = [w for _, w in self.samples if w]
        if mh:
            out.update(sclk_mhz_mean=sum(mh) / len(mh), sclk_mhz_min=min(mh), sclk_mhz_max=max(mh))
        if pw:
            out.update(power_w_mean=sum(pw) / len(pw), power_w_max=max(pw))
        if not self.source:  # one-shot fallback outside sysfs: rocm-smi (slow, so not sampled during the region)
            import shutil
            import subprocess
            smi = shutil.which("rocm-smi")
            if smi:
                try:
                    txt = subprocess.run([smi, "--showclocks", "--showpower"], capture_output=True, text=True, timeout=20).stdout
                    out["rocm_smi_after_region"] = [ln.strip() for ln in txt.splitlines() if "sclk" in ln.lower() or "power" in ln.lower()][:6]
                except Exception as e:
                    out["rocm_smi_error"] = str(e)
        return out


def dropin_leg(local, batch=2, depth=6):
    """The reference's UNCHANGED calling pattern on its own circuit (operator/src/snarks/common.ts:23-29): for every
    proof a new `buildBn128()` object, the provingKeyBin buffer handed over again, a pageable host witness.  First call =
    parse + upload + window tables + proof; steady state = process-level key cache hit + proof."""
    import zkr_hip
    from zkr_hip import rollup
    circ = rollup.RollupCircuit(batch, depth)
    pkb, vk_bin = zkr_hip.setup_r1cs_websnark(circ.r1cs(), device=local)
    privs = [0x5A4B1000 + 7919 * i for i in range(4)]
    state = rollup.RollupState(circ.depth)
    for i, pv in enumerate(privs):
        state.deposit(i, rollup.gen_public_key(pv), 10 ** 20, 0)
    txs = [state.transfer(j % 4, (j + 1) % 4, 10 ** 17, 10 ** 15, privs[j % 4]) for j in range(circ.batch)]
    wb = circ.calculate_witness(circ.flatten_inputs(state.batch_inputs(txs)))
    pub = circ.public_signals(wb)
    zkr_hip.clear_key_cache()
    loads0 = zkr_hip.key_cache_stats["loads"]
    times, proofs = [], []
    for i in range(8):
        t0 = time.perf_counter()
        bn = zkr_hip.build_bn128(local)                       # common.ts:23, per call
        proofs.append(bn.groth16GenProof(wb, pkb))            # common.ts:29 (random blinding, as the reference)
        times.append(1e3 * (time.perf_counter() - t0))
    ok = all(zkr_hip.verify(vk_bin, zkr_hip.proof_bytes_from_json(p), pub) for p in proofs)
    loads = zkr_hip.key_cache_stats["loads"] - loads0
    zkr_hip.clear_key_cache()
    steady = sorted(times[1:])
    return {"circuit": "BatchProcessTx(%d, %d) through the websnark provingKeyBin (%d MB), new Bn128 object per proof" % (batch, depth, len(pkb) >> 20),
            "dropin_first_ms": times[0], "dropin_steady_ms": steady[len(steady) // 2], "key_loads": loads, "proofs_verified": len(proofs) if ok else 0}


def bcast_modes_leg(key, wb, local):
    """Both replication modes of the multi-GPU path timed on ONE GPU, a device-to-device clone standing in for the wire
    (VERDICT r1 item 7b): "full" = whole arena adopted in place; "base" = compact arena + local rebuild of the window
    levels.  wire_ms_at_153GBps = the bytes over one xGMI link, the per-link bound of a ring / chain broadcast."""
    import torch
    from zkr_hip.batch import _tensor_from_ptr
    want = key.prove(wb, 5, 7)
    out = {}
    for mode in ("full", "base"):
        ptr, n = key.arena() if mode == "full" else key.base_arena()
        view = _tensor_from_ptr(ptr, n, local)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        replica = view.clone()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        k2 = zkr_hip_adopt(mode, replica, n, local)
        t2 = time.perf_counter()
        same = k2.prove(wb, 5, 7) == want
        k2.close()
        del replica
        out[mode] = {"bytes": n, "clone_ms": 1e3 * (t1 - t0), "adopt_ms": 1e3 * (t2 - t1), "wire_ms_at_153GBps": n / 153e9 * 1e3,
                     "replica_proof_identical": bool(same)}
    return out


def zkr_hip_adopt(mode, replica, n, local):
    import zkr_hip
    if mode == "full":
        return zkr_hip.ProvingKey.adopt_arena(replica.data_ptr(), n, local, keepalive=replica)
    return zkr_hip.ProvingKey.adopt_base_arena(replica.data_ptr(), n, local)


def tx_circuit_leg(local, steps, batch=2, depth=6):
    """the reference's own tx circuit (tx.circom:3 = BatchProcessTx(2, 6), m = 2^17; or another batch
    size of the same template) end to end on this
    GPU -- native constraint system, Groth16 setup on the device, native witness builder (timed on the host), proofs
    pipelined two deep, every proof checked by the native verifier.  Reported beside the headline line, never as
    `value` (the metric is quoted on the 2^20 configuration)."""
    import torch
    import zkr_hip
    from zkr_hip import rollup
    t0 = time.time()
    circ = rollup.RollupCircuit(batch, depth)
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(circ.r1cs(), device=local)
    setup_s = time.time() - t0
    privs = [0x5A4B1000 + 7919 * i for i in range(8)]
    state = rollup.RollupState(circ.depth)
    for i, pv in enumerate(privs):
        state.deposit(i, rollup.gen_public_key(pv), 10 ** 20, 0)
    n_wit, wits, pubs, wit_ms = 4, [], [], []
    for b in range(n_wit):
        txs = [state.transfer((2 * b + j) % 8, (2 * b + j + 3) % 8, 10 ** 17 * (j + 1), 10 ** 15, privs[(2 * b + j) % 8]) for j in range(circ.batch)]
        flat = circ.flatten_inputs(state.batch_inputs(txs))
        t1 = time.perf_counter()
        wb = circ.calculate_witness(flat)
        wit_ms.append(1e3 * (time.perf_counter() - t1))
        pubs.append(circ.public_signals(wb))
        wits.append(torch.frombuffer(bytearray(wb), dtype=torch.uint8).cuda(local))
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [wits[i % n_wit].data_ptr() for i in range(steps)]
    tw = time.perf_counter()                                    # warm: launch plans, and the device's clocks -- the legs before this
    while time.perf_counter() - tw < 0.4:                       # one run on the host for a minute (CPU baselines), the GPU idles down
        key.prove_batch_device(ptrs[:8], stream=stream)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    proofs = key.prove_batch_device(ptrs, stream=stream)
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    assert zkr_hip.verify_batch(vk_bin, proofs, [pubs[i % n_wit] for i in range(steps)]), "a proof of the tx circuit failed the pairing check"
    ok = steps
    # the reference's own sequence, one batch at a time (createProofGenerator, common.ts:10-53): calculateWitness -> groth16GenProof
    # on the host witness -> isValid, nothing overlapped
    seq = None
    if (batch, depth) == (2, 6):
        parts = [0.0, 0.0, 0.0]
        n_seq = 12
        for it in range(n_seq + 2):
            ta = time.perf_counter()
            wb = circ.calculate_witness(flat)
            tb = time.perf_counter()
            pr = key.prove(wb)
            tc = time.perf_counter()
            good = zkr_hip.verify(vk_bin, pr, circ.public_signals(wb))
            td = time.perf_counter()
            assert good
            if it >= 2:
                parts = [parts[0] + tb - ta, parts[1] + tc - tb, parts[2] + td - tc]
        seq = {"witness_ms": 1e3 * parts[0] / n_seq, "proof_ms": 1e3 * parts[1] / n_seq, "is_valid_ms": 1e3 * parts[2] / n_seq, "total_ms": 1e3 * sum(parts) / n_seq, "calls": n_seq}
    domain = key.info()["domainSize"]
    key.close()
    return {"circuit": "BatchProcessTx(%d, %d)%s" % (circ.batch, circ.depth, " (tx.circom)" if (batch, depth) == (2, 6) else ""), "nVars": circ.n_vars, "nPublic": circ.n_public,
            "nConstraints": circ.n_constraints, "domainSize": domain, "setup_s": setup_s,
            "witness_ms_host": sum(wit_ms) / len(wit_ms), "proofs": steps, "proofs_per_s": steps / el, "ms_per_proof": 1e3 * el / steps,
            "proofs_verified": ok, "facade_sequential": seq}


def size_leg(local, log_m, shape="rollup", steps=6, warmup=2, peak_gmul=None, device_state=None):
    """Another BASELINE.json config on this GPU, beside the headline line: configs[2] (2^22 rollup-shaped, the default leg) or
    configs[4] (2^24 dense random, --with-2-24-dense).  Same measurement as the headline at its size: key computed on the
    device, resident witnesses, `steps` pipelined proofs timed, every one through the native verifier afterwards (the vk
    comes from the setup, not from the proofs), the dominant kernel's roofline by the same formula, and the synchronous
    proof a single awaiting caller sees.  Returns a dict; the caller copies the rates into `config` / `roofline` as scalars."""
    import torch
    import zkr_hip
    zkr_hip.synth_set_shape(1 if shape == "dense" else 0)
    try:
        t0 = time.time()
        key, w0, aux = zkr_hip.ProvingKey.synth(log_m, N_PUBLIC, CIRCUIT_SEED, TOXIC_SEED, device=local, want_aux=True)
        vk_bin = key.synth_vk(aux)
        del aux
        wits = [torch.frombuffer(bytearray(w0), dtype=torch.uint8).cuda(local),
                torch.frombuffer(bytearray(zkr_hip.synth_witness(log_m, N_PUBLIC, CIRCUIT_SEED, CIRCUIT_SEED + 1)), dtype=torch.uint8).cuda(local)]
        del w0
        setup_s = time.time() - t0
        info = key.info()
        stream = torch.cuda.current_stream().cuda_stream
        run = lambda first, count: key.prove_batch_device([wits[i % 2].data_ptr() for i in range(first, first + count)],
                                                          [3000003 + i for i in range(first, first + count)],
                                                          [4000003 + i for i in range(first, first + count)], stream)
        run(0, warmup)
        key.prof_enable(True)
        key.prof_reset()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        proofs = run(0, steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t1
        prof = key.prof()
        key.prof_enable(False)
        pubs = [public_signals_of(w) for w in wits]
        verify_timed_proofs(vk_bin, proofs, lambda i: pubs[i % 2])
        roofline, _ = roofline_record(key, info, prof, el / steps, device_state, log_m, shape, local, peak_gmul=peak_gmul)
        key.prove_device(wits[0].data_ptr(), r=5, s=7, stream=stream)
        t1 = time.perf_counter()
        for i in range(3):
            key.prove_device(wits[i % 2].data_ptr(), r=21 + i, s=23 + i, stream=stream)
        sync_ms = 1e3 * (time.perf_counter() - t1) / 3
        arena = key.arena()[1]
        key.close()
        return {"workload": "2^%d-constraint synthetic %s" % (log_m, "rollup circuit" if shape == "rollup" else "dense random R1CS"),
                "proofs": steps, "proofs_per_s": steps / el, "ms_per_proof": 1e3 * el / steps, "sync_latency_ms": sync_ms, "proofs_verified": steps,
                "setup_s": setup_s, "arena_bytes": arena, "nVars": info["nVars"], "nnzA": info["nnzA"], "nnzB": info["nnzB"],
                "roofline": {k: v for k, v in roofline.items() if k not in ("streaming", "note")},
                "stage_ms_per_proof": {k: v[0] / steps for k, v in prof.items()}}
    finally:
        zkr_hip.synth_set_shape(0)


def withdraw_leg(local, steps=256):
    """The reference's MOST-CALLED proof (operator/src/snarks/withdraw.ts:6-10 = createProofGenerator on withdraw.circom; five call
    sites in contracts/__tests__/rollup.test.ts:105,179,208,233,295): Withdraw() through the same three forms as the tx circuit --
    one awaited proof from a host witness (what `genWithdrawVerifierProof` awaits), the reference's unchanged drop-in call
    (new Bn128 object + provingKeyBin per proof: key cache), and fused batches of resident witnesses.  Every proof verified."""
    import torch
    import zkr_hip
    from zkr_hip import rollup
    circ = rollup.WithdrawCircuit()
    r1cs = circ.r1cs()
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(r1cs, device=local)
    pkb, vk_bin2 = zkr_hip.setup_r1cs_websnark(r1cs, device=local)
    privs = [0x5A4B2000 + 104729 * i for i in range(8)]
    t1 = time.perf_counter()
    wbs = [circ.calculate_witness({"privateKey": rollup.format_priv_key(pv), "nullifier": 1000 + i}) for i, pv in enumerate(privs)]
    wit_ms = 1e3 * (time.perf_counter() - t1) / len(privs)
    pubs = [circ.public_signals(wb) for wb in wbs]
    info = key.info()
    # (1) one awaited proof at a time from a host buffer
    for i in range(4):
        key.prove(wbs[i % 8])
    times, single = [], []
    for i in range(24):
        t1 = time.perf_counter()
        single.append(key.prove(wbs[i % 8]))
        times.append(1e3 * (time.perf_counter() - t1))
    ok = zkr_hip.verify_batch(vk_bin, single, [pubs[i % 8] for i in range(24)])
    single_ms = sorted(times)[len(times) // 2]
    # (2) the reference's sequence: calculateWitness -> groth16GenProof -> isValid (common.ts:15-38)
    parts = [0.0, 0.0, 0.0]
    n_seq = 12
    for it in range(n_seq):
        ta = time.perf_counter()
        wb = circ.calculate_witness({"privateKey": rollup.format_priv_key(privs[it % 8]), "nullifier": 1000 + it % 8})
        tb = time.perf_counter()
        pr = key.prove(wb)
        tc = time.perf_counter()
        ok = zkr_hip.verify(vk_bin, pr, circ.public_signals(wb)) and ok
        td = time.perf_counter()
        parts = [parts[0] + tb - ta, parts[1] + tc - tb, parts[2] + td - tc]
    # (3) fused batches of resident witnesses
    d_w = [torch.frombuffer(bytearray(wb), dtype=torch.uint8).cuda(local) for wb in wbs]
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [d_w[i % 8].data_ptr() for i in range(steps)]
    key.prove_batch_device(ptrs[:32], stream=stream)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    fused = key.prove_batch_device(ptrs, stream=stream)
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    ok = zkr_hip.verify_batch(vk_bin, fused, [pubs[i % 8] for i in range(steps)]) and ok
    key.close()
    # (4) the unchanged caller: new Bn128 + the provingKeyBin buffer per proof
    zkr_hip.clear_key_cache()
    dt, dp = [], []
    for i in range(8):
        t1 = time.perf_counter()
        bn = zkr_hip.build_bn128(local)
        dp.append(bn.groth16GenProof(wbs[i], pkb))
        dt.append(1e3 * (time.perf_counter() - t1))
    ok = all(zkr_hip.verify(vk_bin2, zkr_hip.proof_bytes_from_json(p), pubs[i]) for i, p in enumerate(dp)) and ok
    zkr_hip.clear_key_cache()
    steady = sorted(dt[1:])
    if not ok:
        raise SystemExit("a proof of the withdraw circuit failed the pairing check")
    return {"circuit": "Withdraw() (withdraw.circom)", "nVars": info["nVars"], "domainSize": info["domainSize"], "nPublic": circ.n_public,
            "witness_ms_host": wit_ms, "single_proof_ms": single_ms, "fused_proofs_per_s": steps / el, "fused_ms_per_proof": 1e3 * el / steps,
            "dropin_first_ms": dt[0], "dropin_steady_ms": steady[len(steady) // 2],
            "sequence_ms": {"witness": 1e3 * parts[0] / n_seq, "proof": 1e3 * parts[1] / n_seq, "is_valid": 1e3 * parts[2] / n_seq, "total": 1e3 * sum(parts) / n_seq},
            "proofs_verified": 24 + n_seq + steps + 8}


def facade_pipeline_leg(local, n_batches=256, chunk=64, witness="gpu"):
    """The whole of createProofGenerator (operator/src/snarks/common.ts:10-53) for a stream of rollup batches of the
    reference's tx circuit, every step native and overlapped: witness (`calculateWitness`, :15-17) -> proof
    (`groth16GenProof`, :29) -> acceptance (`isValid`, :30-34: zkr_verify_batch, one merged pairing product per chunk).
    witness="gpu": zkr_rollup_witness_batch_device builds a chunk's witnesses on the GPU (one thread per transaction) and
    leaves them in HBM for zkr_prove_batch_device, while the previous chunk is being proved; witness="host": the host
    builder on a pool of threads and zkr_prove_batch on pageable host witnesses.  End-to-end rate over n_batches distinct
    batches (consecutive states of one rollup), circuit inputs prepared beforehand (the operator's side: signing, tree
    updates)."""
    import queue
    import threading
    from concurrent.futures import ThreadPoolExecutor
    import zkr_hip
    from zkr_hip import rollup
    circ = rollup.RollupCircuit(2, 6)
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(circ.r1cs(), device=local)
    privs = [0x5A4B1000 + 7919 * i for i in range(8)]
    state = rollup.RollupState(circ.depth)
    for i, pv in enumerate(privs):
        state.deposit(i, rollup.gen_public_key(pv), 10 ** 24, 0)
    flats = []
    for b in range(n_batches):
        txs = [state.transfer((2 * b + j) % 8, (2 * b + j + 3) % 8, 10 ** 15 * (j + 1) + b, 10 ** 12, privs[(2 * b + j) % 8]) for j in range(circ.batch)]
        flats.append(circ.flatten_inputs(state.batch_inputs(txs)))
    workers = max(2, effective_host_cores() - 2)
    w0 = circ.calculate_witness(flats[0])
    key.prove_batch([w0] * 4)                                   # warm: staging buffers, fused launch plans
    if witness == "gpu":  # warm: the builder's tables, and torch's first device-to-host copy (tens of milliseconds once per process)
        circ.calculate_witness_batch_device(flats[:2], device=local)[:, 32:64].cpu()
    verified = [0]
    verified_lock = threading.Lock()
    failures = []
    trace = [] if os.environ.get("ZKR_PIPE_TRACE") else None
    q_verify, q_wit = queue.Queue(), queue.Queue(maxsize=2)
    n_pub = circ.n_public

    def verifier():
        while True:
            item = q_verify.get()
            if item is None:
                return
            proofs, pubs = item
            ta = time.perf_counter()
            if not isinstance(pubs, list):                           # the witnesses' public heads, still on the device
                head = pubs.cpu().numpy()
                pubs = [[int.from_bytes(row[32 * j:32 * j + 32].tobytes(), "little") for j in range(n_pub)] for row in head]
            try:
                good = zkr_hip.verify_batch(vk_bin, proofs, pubs)
            except Exception as e:  # a verifier thread must keep draining its queue: the producer would block otherwise
                good = False
                sys.stderr.write("facade pipeline: verification raised %r\n" % (e,))
            with verified_lock:       # eight threads: += on a shared cell is a read-modify-write across a len() call
                if good:
                    verified[0] += len(proofs)
                else:
                    failures.append(len(proofs))
            if trace is not None:
                trace.append(("V%d" % len(proofs), ta, time.perf_counter()))

    # chunk plan: the GPU builder's latency is flat (~30 ms whatever the count, ~60 ms beside a running prover), so it is called
    # TWICE: for the first `chunk` batches (the prover starts after one builder latency) and for all the others, built while
    # the first ones are proved (64 proofs take longer than the second call; with a second call of 64 after a first of 32 the
    # prover waited 25 ms for it).  The prover takes the witnesses in pieces of `chunk` (calls of that size keep its pipeline
    # full) and verification streams behind the proofs in pieces of 16 on four host threads.  ZKR_PIPE_HOST_FIRST=n: the first
    # n batches from the HOST builder on the thread pool while the GPU builds its first chunk.
    host_first = min(int(os.environ.get("ZKR_PIPE_HOST_FIRST", "0")), n_batches) if witness == "gpu" else 0
    sizes, left = [], n_batches - host_first
    if left > 0:
        sizes.append(min(chunk, left))
        left -= sizes[-1]
    if left > 0:
        sizes.append(left)

    def gpu_witnesses():                                            # chunk i + 1 is built while chunk i is proved
        import torch
        torch.cuda.set_device(local)
        c0 = host_first
        for sz in sizes:
            ta = time.perf_counter()
            t = circ.calculate_witness_batch_device(flats[c0:c0 + sz], device=local)
            if trace is not None:
                trace.append(("W%d" % sz, ta, time.perf_counter()))
            q_wit.put(t)
            c0 += sz
        q_wit.put(None)

    t0 = time.perf_counter()
    # 0.75 ms of one core per proof; with the GPU builder the host is idle: pieces of 8 on eight threads, so the tail after the
    # last proof is short; beside the host builder's pool four threads and pieces of 16 (eight cost it 15 %: 499 against 583)
    n_ver, piece_ver = (8, 8) if witness == "gpu" else (4, 16)
    vts = [threading.Thread(target=verifier) for _ in range(n_ver)]
    for vt in vts:
        vt.start()
    def to_verify(proofs, pubs):
        for o in range(0, len(proofs), piece_ver):
            q_verify.put((proofs[o:o + piece_ver], pubs[o:o + piece_ver]))

    try:
        if witness == "gpu":
            wt = threading.Thread(target=gpu_witnesses)
            wt.start()
            if host_first:
                with ThreadPoolExecutor(min(workers, host_first)) as pool:
                    wits = list(pool.map(circ.calculate_witness, flats[:host_first]))
                ta = time.perf_counter()
                proofs = key.prove_batch(wits)
                if trace is not None:
                    trace.append(("Ph%d" % len(proofs), ta, time.perf_counter()))
                to_verify(proofs, [circ.public_signals(w) for w in wits])
            while True:
                t = q_wit.get()
                if t is None:
                    break
                for o in range(0, t.shape[0], chunk):
                    ta = time.perf_counter()
                    piece = t[o:o + chunk]
                    proofs = key.prove_batch_device([piece[i].data_ptr() for i in range(piece.shape[0])])     # random blinding, as the reference draws it
                    tb = time.perf_counter()
                    if trace is not None:
                        trace.append(("P%d" % len(proofs), ta, tb))
                    to_verify(proofs, piece[:, 32:32 * (n_pub + 1)])      # the verifier threads fetch the public signals (2.3 KB per proof)
                del t
            wt.join()
        else:
            with ThreadPoolExecutor(workers) as pool:
                futs = [pool.submit(circ.calculate_witness, f) for f in flats]          # ctypes releases the GIL inside the builder
                for c0 in range(0, n_batches, chunk):
                    wits = [f.result() for f in futs[c0:c0 + chunk]]
                    proofs = key.prove_batch(wits)
                    to_verify(proofs, [circ.public_signals(w) for w in wits])
    finally:                      # whatever the prover or a builder raised: the verifier threads end (they only stop on the sentinel)
        for vt in vts:
            q_verify.put(None)
        for vt in vts:
            vt.join()
    el = time.perf_counter() - t0
    key.close()
    if verified[0] != n_batches or failures:
        raise SystemExit("facade pipeline: %d of %d proofs verified, %d failing pieces" % (verified[0], n_batches, len(failures)))
    if trace:
        for name, ta, tb in sorted(trace, key=lambda e: e[1]):
            sys.stderr.write("%-6s %7.1f -> %7.1f  (%.1f ms)\n" % (name, 1e3 * (ta - t0), 1e3 * (tb - t0), 1e3 * (tb - ta)))
    return {"circuit": "BatchProcessTx(2, 6) (tx.circom)", "batches": n_batches, "chunk": chunk, "chunks": (([["host", host_first]] if host_first else []) + sizes) if witness == "gpu" else None,
            "witness": "GPU builder (zkr_rollup_witness_batch_device), witnesses stay in HBM" if witness == "gpu" else "host builder on %d threads" % workers,
            "end_to_end_proofs_per_s": n_batches / el, "ms_per_batch": 1e3 * el / n_batches, "proofs_verified": verified[0],
            "verification_failures": len(failures),
            "steps": "witness -> proof -> zkr_verify_batch, overlapped (chunk i + 1's witnesses under chunk i's proofs, verification on host threads)"}


def self_launch(n_gpus):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a CHILD `python -m torch.distributed.run`
    (one process per GPU, rendezvous on 127.0.0.1 at a free port) with this command line, relay rank 0's single JSON
    line on stdout and return the child's exit code.  Nothing in this parent touches HIP or torch.cuda -- a process
    that has initialised the GPU must never exec or fork the ranks."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # the host driver only supports dmabuf IPC (RCCL across processes)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = []
    for ln in child.stdout:  # stderr goes straight through; stdout is filtered down to the result line
        if ln.startswith("{"):
            lines.append(ln.rstrip("\n"))
        else:
            sys.stderr.write(ln)
    rc = child.wait()
    for ln in lines:
        print(ln, flush=True)
    if rc == 0 and len(lines) != 1:
        sys.stderr.write("bench.py: expected one JSON line from rank 0, got %d\n" % len(lines))
        return 1
    return rc


def roofline_record(key, info, prof, per_proof_s, device_state, log_m, shape, local, peak_gmul=None):
    """The `roofline` object of the line: the dominant kernel's algorithmic bytes per launch -- every base
    point and every scalar of the MSM read once (64 B G1 / 128 B G2 point + 32 B scalar) -- over its average
    launch duration (hipEvents around every launch, on the stream it is launched on: zkr_prof_*), against the HBM peak; the
    VALU bound that really binds it beside it.  Returns (roofline, hbm_whole_proof or None)."""
    import zkr_hip
    g1_pts = info["ptsA"] + info["ptsB1"] + info["ptsC"] + info["ptsH"]
    win = key.windows()  # K mixed additions per point (one per window level of the key table)
    # launches of the G1 accumulation per proof: 2 since round 6 (B1 + A + C in ONE launch, then H), 4 before -- taken from the
    # profile itself (one ingest_kernel launch per proof), so `achieved` stays bytes of ONE launch over the duration of ONE launch
    proofs_profiled = max(prof.get("ingest", (0.0, 0))[1], 1)
    g1_lpp = max(prof["msm_accum_g1"][1] / proofs_profiled, 1e-9)
    cands = {
        "msm_accum_kernel<Fq>": ("msm_accum_g1", 96.0 * g1_pts / g1_lpp, MADD_G1 * g1_pts / g1_lpp * win["A"][1]),
        "msm_accum_kernel<Fq2>": ("msm_accum_g2", 160.0 * info["ptsB2"], MADD_G2 * info["ptsB2"] * win["B2"][1]),
    }
    dom, best = None, -1.0
    for name, (st, _, _) in cands.items():
        if prof[st][0] > best:
            dom, best = name, prof[st][0]
    st, bytes_per_launch, fqmul_per_launch = cands[dom]
    ms_total, launches = prof[st]
    avg_ms = ms_total / max(launches, 1)
    achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9
    traffic, traffic_src, proof_traffic, pmc_file = None, "no PMC pass of round %d under profiles/ (%s): traffic is not carried over from older kernels" % (ROUND, PMC_FILE), None, PMC_FILE
    census_busy, census_src = None, None
    try:  # HBM bytes per launch from the committed PMC passes (bench.py cannot collect PMCs itself) -- THIS round's only: an older
          # file describes older kernels
        pmc = json.load(open(os.path.join(ROOT, "profiles", pmc_file)))
        if pmc.get("round") != ROUND:
            raise ValueError("stale PMC file")
        if pmc["config"]["log_m"] == log_m and shape == "rollup":
            # whole proof: every kernel of the proving path (not key build), per ingest_kernel launch = per proof
            skip = ("precompute", "fixed_base", "twiddle", "gather", "fq_mul_bench", "rocclr_copy")
            per_run = sum(v["hbm_bytes_per_launch"] * v["launches"] for k, v in pmc["kernels"].items() if not any(x in k for x in skip))
            proof_traffic = per_run / pmc["kernels"]["ingest_kernel"]["launches"]
            traffic = pmc["kernels"][dom]["hbm_bytes_per_launch"]
            # (short first: the driver's record keeps 120 characters of a string)
            traffic_src = "profiles/%s: FETCH_SIZE x %.3f (calibrated on %s) + WRITE_SIZE, separate --pmc passes, %s; calibration: %s" % (
                pmc_file, pmc["calibration"][pmc["kernels"][dom]["pattern"]], pmc["kernels"][dom]["pattern"], pmc.get("schedule", "isolated kernels"), pmc["calibration_source"])
    except Exception:
        pass
    # the kernels of the path that STREAM (SURVEY 8(d) regime 1), each against the HBM peak: algorithmic bytes per launch
    # over the launch's own duration (hipEvents around every launch, two proofs in flight: the kernels share the chip
    # with the accumulations; isolated durations are in profiles/)
    m_, n_ = info["domainSize"], info["nVars"]
    # round 4: one spmv_kernel launch evaluates BOTH sides of the QAP and one ntt_pass_kernel launch runs a pass of TWO transforms
    stream_bytes = {"ingest": ("ingest_kernel", 64.0 * n_), "spmv_a": ("spmv_kernel (A and B sides)", 36.0 * (info["nnzA"] + info["nnzB"]) + 64.0 * n_ + 64.0 * m_),
                    "ntt_pass": ("ntt_pass_kernel (a pass of two transforms)", 128.0 * m_), "combine_h": ("combine_h_kernel", 96.0 * m_)}
    streaming = {}
    for st_name, (kname, nbytes) in stream_bytes.items():
        ms_t, nl = prof.get(st_name, (0.0, 0))
        if nl:
            gbps = nbytes / (ms_t / nl * 1e-3) / 1e9
            streaming[kname] = {"algorithmic_bytes_per_launch": nbytes, "avg_launch_us": 1e3 * ms_t / nl, "launches": nl,
                                "achieved_GBps": gbps, "frac_of_hbm_peak": gbps / HBM_PEAK_GBPS}
    roofline = {"bound": "hbm", "binding_bound": "valu", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "streaming": streaming,
                "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_src,
                "avg_launch_ms": avg_ms, "launches": launches, "launches_per_proof": launches / proofs_profiled,
                "algorithmic_bytes_per_launch": bytes_per_launch,
                "note": "Pippenger bucket accumulation is integer-VALU bound (v_mad_u64_u32), not HBM bound; see valu. traffic > algorithmic bytes by design: "
                        "the kernel gathers one precomputed 64-byte multiple per window (13 per point, 832 B) instead of re-deriving it, "
                        "plus the 4-byte entries; traffic = FETCH_SIZE x the factor calibrated on random 64-byte gathers + WRITE_SIZE (traffic_source). "
                        "avg_launch_ms is measured with two proofs in flight (the kernel shares the chip with the other streams); isolated it runs 0.76 ms"}
    try:
        legacy = None
        if peak_gmul is None:
            peak_gmul = zkr_hip.bench_fq_mul(local)
            legacy = zkr_hip.bench_fq_mul(local, legacy=True)
        gm = fqmul_per_launch / (avg_ms * 1e-3) / 1e9
        roofline["valu"] = {"bound": "valu", "peak_fq_mul_per_s_G": peak_gmul, "unit": "G Fq-mul/s (162 mad32 each: 9 x 29-bit limbs, no carry words)",
                            "peak_fq_mul_per_s_G_legacy_8x32": legacy,
                            "achieved_fq_mul_per_s_G": gm, "frac": gm / peak_gmul,
                            "window_bits": win["A"][0], "additions_per_point": win["A"][1]}
        # the same rate against the chip's own bound, not only against this library's multiplier:
        # a product needs 162 v_mad_u64_u32, an instruction that issues at 16 lanes per clock (4 cycles per wave64,
        # tools/valu_clock.hip) on each of the 1024 SIMDs (256 CUs x 4), so at clock f no multiplier of this form can
        # exceed 1024 * 16 * f / 162 -- quoted at the clock SAMPLED during the timed region and at the 2.4 GHz boost
        # clock.  The column bookkeeping (shifts, masks, the m_k products: ~60 of ~222 instructions) is what
        # separates the microbenchmark from this bound; the 8 x 32-bit form needs 136 multiply-adds but 136 carry
        # additions at the same 4 cycles on top (its own bound would be 1024 * 16 * f / 136 = 285 G/s at 2.36 GHz,
        # of which it reaches 0.46).
        mhz = (device_state or {}).get("sclk_mhz_mean")
        bound = lambda f_mhz: 1024 * 16 * f_mhz * 1e6 / MADS_PER_MUL / 1e9
        roofline["valu"]["mad_only_bound"] = {
            "sampled_sclk_mhz": mhz,
            "bound_at_sampled_clock_G": bound(mhz) if mhz else None, "frac_at_sampled_clock": gm / bound(mhz) if mhz else None,
            "bound_at_2400_mhz_G": bound(2400.0), "frac_at_2400_mhz": gm / bound(2400.0),
            "microbench_over_bound_at_sampled_clock": peak_gmul / bound(mhz) if mhz else None}
        # whole proof: every field multiplication of the path (Fq and Fr cost the same) over the time per proof.
        # mixed addition MADD_G1 / MADD_G2 per table entry (in units of one hot-path multiplication, see the constants at the top; the NTT and QAP products are the 8 x 32-bit kind, counted one for one); NTT: 6 transforms of (m/2) log2 m butterflies + 5m
        # element-wise products; QAP rows: one per non-zero; bucket reduction: 2 full additions (ADD_G1 / ADD_G2) per
        # bucket + the group sums (about 8 per group of 32 buckets), three G1 bucket sets (C and H share one) and the G2 one
        m, lg = info["domainSize"], info["domainSize"].bit_length() - 1
        nb = 1 << (win["A"][0] - 1)
        n_red_g1 = 3 if win["C"] == win["H"] else 4   # C and H share one bucket set and ONE reduction when their geometry agrees (round 3)
        red = (2 * nb + 8 * (nb >> 5)) * (ADD_G1 * n_red_g1 + ADD_G2)
        total_mul = (MADD_G1 * g1_pts * win["A"][1] + MADD_G2 * info["ptsB2"] * win["B2"][1] + 6 * (m // 2) * lg + 5 * m
                     + info["nnzA"] + info["nnzB"] + red)
        gw = total_mul / per_proof_s / 1e9
        roofline["valu"]["whole_proof"] = {"fq_mul_per_proof": total_mul, "achieved_fq_mul_per_s_G": gw, "frac": gw / peak_gmul}
        # the same as SCALARS of `roofline` (the driver's record keeps scalars and short strings of this object, not nested ones):
        # *_kernel = the dominant kernel in flight, *_proof = every field multiplication of the proof over the time per proof;
        # valu_frac_* against the in-process multiplier microbenchmark, mad_bound_frac_* against 1024 SIMDs x 16 lanes x clock / 162
        roofline.update({"valu_peak_fq_mul_G": peak_gmul, "valu_fq_mul_G_kernel": gm, "valu_fq_mul_G_proof": gw,
                         "valu_frac_kernel": gm / peak_gmul, "valu_frac_proof": gw / peak_gmul,
                         "mad_bound_frac_kernel": gm / bound(mhz) if mhz else None, "mad_bound_frac_proof": gw / bound(mhz) if mhz else None,
                         "sclk_mhz_sampled": mhz})
    except Exception as e:  # microbench is informative only
        roofline["valu"] = {"error": str(e)}
    # ratios the record should carry itself: measured HBM traffic over algorithmic bytes, kernel and proof
    roofline["traffic_over_algorithmic"] = (traffic / bytes_per_launch) if traffic else None
    # VALU-busy fraction of the timed step by COUNTERS: SQ_INSTS_VALU of every kernel of a proof (isolated pass: dispatch-mode counters
    # serialise anyway; SQ_ACTIVE_INST_VALU charges one quad-cycle per instruction) x 4 cycles / (1024 SIMDs x sampled clock x step)
    try:
        cen = json.load(open(os.path.join(ROOT, "profiles", CENSUS_FILE)))
        mhz = (device_state or {}).get("sclk_mhz_mean")
        if cen.get("round") == ROUND and cen["config"]["log_m"] == log_m and shape == "rollup" and mhz:
            roofline["valu_busy_step"] = 4.0 * cen["valu_wave_instructions_per_proof"] / (1024 * mhz * 1e6 * per_proof_s)
            roofline["valu_wave_instructions_per_proof"] = cen["valu_wave_instructions_per_proof"]
            roofline["valu_busy_source"] = "profiles/%s (rocprofv3 --pmc SQ_INSTS_VALU ..., isolated kernels) x 4 cycles / (1024 SIMDs x sclk sampled in this run x ms_per_step)" % CENSUS_FILE
    except Exception:
        pass
    whole = None if proof_traffic is None else {
        "bytes_per_proof": proof_traffic, "GBps_per_gpu": proof_traffic / per_proof_s / 1e9,
        "frac_of_peak": proof_traffic / per_proof_s / 1e9 / HBM_PEAK_GBPS,
        "source": "sum over the proving kernels of profiles/%s (FETCH_SIZE x the factor calibrated per access pattern + WRITE_SIZE)" % pmc_file}
    if whole:
        # B_proof = B_spmv + B_ntt + B_msm, every base point, scalar, QAP entry and vector element once
        n_, m_, p_ = info["nVars"], info["domainSize"], N_PUBLIC
        b_proof = (36.0 * (info["nnzA"] + info["nnzB"]) + 32.0 * n_ + 64.0 * m_) + 576.0 * m_ + (
            64.0 * (info["ptsA"] + info["ptsB1"] + info["ptsC"] + info["ptsH"]) + 128.0 * info["ptsB2"] + 32.0 * n_ + 32.0 * m_)
        whole["algorithmic_bytes_per_proof"] = b_proof
        roofline.update({"hbm_traffic_GB_per_proof": whole["bytes_per_proof"] / 1e9, "hbm_traffic_frac_proof": whole["frac_of_peak"],
                         "algorithmic_GB_per_proof": b_proof / 1e9, "hbm_traffic_over_algorithmic_proof": whole["bytes_per_proof"] / b_proof})
    for k, v in streaming.items():   # the streaming kernels' fractions of the HBM peak as scalars: hbm_frac_ingest, _spmv, _ntt_pass, _combine_h
        roofline["hbm_frac_" + k.split("_kernel")[0].split(" ")[0]] = v["frac_of_hbm_peak"]
    return roofline, whole


def shard_leg(key, d_wit, parts, want_proof, local):
    """Intra-proof sharding on ONE GPU (BASELINE configs[2] and [4] are single proofs): the key is cut into
    `parts` shards side by side on this device, every shard's share of one proof runs ALONE (synchronously, one after the
    other), and the slowest share + the host combination is what a proof would take with one shard per GPU -- a PROJECTION
    (no xGMI, no second device involved: the shards exchange nothing but 640 bytes each at the end), labelled as such.
    The combined proof must be the bytes of the whole key's proof."""
    import zkr_hip
    whole = key.prove_device(d_wit.data_ptr(), r=1000003, s=2000003)
    t1 = time.perf_counter()
    for i in range(3):
        key.prove_device(d_wit.data_ptr(), r=1000003, s=2000003)
    whole_ms = 1e3 * (time.perf_counter() - t1) / 3
    # one shard at a time (built, timed, released): on a real node every GPU holds ONE shard; eight of a 2^24 key side by side
    # beside the whole key would not fit one GPU's 288 GB
    rows, partials, build_s = [], [], 0.0
    m_ = key.info()["domainSize"]
    split_ok = parts in (2, 4, 8) and m_ // (parts * parts) >= 64       # zkr_prove_sharded splits calcH over such shards (zkr_multi.hip run_sharded)
    for i in range(parts):
        t1 = time.perf_counter()
        sh = key.shard(i, parts, device=local)
        build_s += time.perf_counter() - t1
        sh.prove_partial_device(d_wit.data_ptr())                       # warm: launch plans, staging
        t1 = time.perf_counter()
        for _ in range(3):
            part = sh.prove_partial_device(d_wit.data_ptr())
        ms = 1e3 * (time.perf_counter() - t1) / 3
        partials.append(part)
        inf = sh.info()
        sh.prof_enable(True)                                            # stage sums of one more run (hipEvents around every launch)
        sh.prof_reset()
        sh.prove_partial_device(d_wit.data_ptr())
        stages = {k: round(v[0], 3) for k, v in sh.prof().items() if v[1]}
        sh.prof_enable(False)
        row = {"part": sh.shard_info()["part"], "ms": ms, "arena_bytes": sh.arena()[1], "points": sum(inf[t] for t in ("ptsA", "ptsB1", "ptsB2", "ptsC", "ptsH")),
               "stage_ms": stages}
        if split_ok:                                                    # the shard's share when calcH is split over the shards, alone on the GPU
            sh.bench_split_solo(d_wit.data_ptr())
            row["split_calch_solo_ms"] = sorted(sh.bench_split_solo(d_wit.data_ptr()) for _ in range(3))[1]
        rows.append(row)
        sh.close()
    t1 = time.perf_counter()
    proof = key.prove_combine(partials, 1000003, 2000003)
    combine_ms = 1e3 * (time.perf_counter() - t1)
    same = proof == whole and (want_proof is None or proof == want_proof)
    if not same:
        raise SystemExit("the sharded proof differs from the whole key's proof")
    slowest = max(r["ms"] for r in rows)
    split = None
    if split_ok:
        # What zkr_prove_sharded does with these shards on a node: calcH split over them (csrc/zkr_prove.hip calc_h_split).  MEASURED
        # here: every shard's share alone on the GPU with its own buffers standing in for the others' (zkr_bench_shard_split_solo)
        # and, separately, the whole sharded proof with all shards concurrently on this one GPU (same bytes as the whole key's).
        # MODELLED: the exchange -- in the cross passes a shard reads 6 and writes 4 vector-columns-of-every-block, (P - 1) / P of
        # them in other GPUs' memory, over 7 xGMI links at once at an ASSUMED half of 153 GB/s each -- and 4 host barriers of 50 us.
        solo = max(r["split_calch_solo_ms"] for r in rows)
        remote_bytes = 10 * (m_ // parts) * 32 * (parts - 1) / parts
        exchange_ms = 1e3 * remote_bytes / (7 * 153e9 * 0.5)
        barriers_ms = 4 * 0.05
        shards_all, agg_ms, agg_rep_ms, same_split, all_form = [], None, None, None, None
        try:                                                            # all shards side by side: may not fit beside the whole key at 2^24
            for i in range(parts):
                shards_all.append(key.shard(i, parts, device=local))
            ptrs = [d_wit.data_ptr()] * parts
            same_split = zkr_hip.prove_sharded_device(shards_all, ptrs, 1000003, 2000003) == whole and zkr_hip.sharded_split_stats() is not None
            all_form = zkr_hip.sharded_last_form()
            t1 = time.perf_counter()
            for _ in range(3):
                zkr_hip.prove_sharded_device(shards_all, ptrs, 1000003, 2000003)
            agg_ms = 1e3 * (time.perf_counter() - t1) / 3
            os.environ["ZKR_SHARD_SPLIT_H"] = "0"
            try:
                zkr_hip.prove_sharded_device(shards_all, ptrs, 1000003, 2000003)
                t1 = time.perf_counter()
                for _ in range(3):
                    zkr_hip.prove_sharded_device(shards_all, ptrs, 1000003, 2000003)
                agg_rep_ms = 1e3 * (time.perf_counter() - t1) / 3
            finally:
                del os.environ["ZKR_SHARD_SPLIT_H"]
        except zkr_hip.ZkrError as e:
            sys.stderr.write("shard leg: all shards side by side: %s\n" % e)
        finally:
            for sh in shards_all:
                sh.close()
        if same_split is False:
            raise SystemExit("the sharded proof with a split calcH differs from the whole key's proof")
        lat = solo + combine_ms + exchange_ms + barriers_ms
        split = {"slowest_shard_solo_ms": solo, "modelled_exchange_ms": exchange_ms, "modelled_barriers_ms": barriers_ms,
                 "remote_bytes_per_shard": remote_bytes, "assumed_link_efficiency": 0.5,
                 "projected_latency_ms": lat, "projected_speedup": whole_ms / lat,
                 "all_shards_on_this_gpu_ms_per_proof": agg_ms, "all_shards_on_this_gpu_ms_per_proof_replicated_calch": agg_rep_ms,
                 "proof_identical_to_whole_key": same_split, "all_shards_form": all_form and all_form["form"], "all_shards_reason": all_form and all_form["reason"],
                 "note": "compute MEASURED (a shard alone; all shards together on one GPU), exchange and barriers MODELLED: no multi-GPU node was available"}
    return {"parts": parts, "measured": False, "whole_key_sync_proof_ms": whole_ms, "per_shard": rows, "slowest_shard_ms": slowest, "combine_ms": combine_ms,
            "projected_latency_ms_one_shard_per_gpu": slowest + combine_ms, "projected_speedup": whole_ms / (slowest + combine_ms),
            "split_calch": split,
            "shard_build_s": build_s, "proof_identical_to_whole_key": True,
            "note": "PROJECTED: shards measured one at a time on one GPU; every shard computes its part of h itself (the first four of calcH's six transforms in full, the last two on its range), so the exchange is 640 B per shard"}


def shards_share_a_gpu(devices, bus_ids):
    """True unless every shard sat on a PHYSICAL GPU of its own: distinct device ordinals AND distinct PCI bus ids
    (zkr_device_pci_bus_id) -- only then is a sharded timing a measurement (`sharded_measured`), otherwise it is a rehearsal."""
    return len(set(devices)) < len(devices) or len(set(bus_ids)) < len(bus_ids) or any(not b for b in bus_ids)


def sharded_multi_leg(key, wit_bytes, devices, r=1000003, s_=2000003, reps=5):
    """ONE proof over SEVERAL devices, MEASURED: shard i of the key on devices[i], the
    full witness resident on each, zkr_prove_sharded_device timed as a caller sees it -- host threads, barriers, the cross passes
    through the other devices' memory, the combination.  Reports which form ran (split / replicated calcH) and why
    (zkr_prove_sharded_last_form), the split's per-phase host milliseconds per shard, the remote GB/s of its cross phases, and
    the same proof with every shard computing h for itself (ZKR_SHARD_SPLIT_H=0).  devices may repeat (rehearsal on one GPU:
    labelled, never a scaling number).  The proof must be the whole key's bytes."""
    import torch
    import zkr_hip
    parts = len(devices)
    bus_ids = [zkr_hip.device_pci_bus_id(d).lower() for d in devices]
    rehearsal = shards_share_a_gpu(devices, bus_ids)
    dev0 = key.device
    d0 = torch.frombuffer(bytearray(wit_bytes), dtype=torch.uint8).to(torch.device("cuda", dev0))
    torch.cuda.synchronize(dev0)
    whole = key.prove_device(d0.data_ptr(), r=r, s=s_)
    t1 = time.perf_counter()
    for _ in range(3):
        key.prove_device(d0.data_ptr(), r=r, s=s_)
    whole_ms = 1e3 * (time.perf_counter() - t1) / 3
    t1 = time.perf_counter()
    shards = [key.shard(i, parts, device=d) for i, d in enumerate(devices)]
    build_s = time.perf_counter() - t1
    out = {"parts": parts, "devices": list(devices), "device_pci_bus_ids": bus_ids, "measured": True, "rehearsal_on_one_gpu": rehearsal, "whole_key_sync_proof_ms": whole_ms, "shard_build_s": build_s,
           "shard_arena_bytes": [sh.arena()[1] for sh in shards]}
    try:
        dws = [torch.frombuffer(bytearray(wit_bytes), dtype=torch.uint8).to(torch.device("cuda", d)) for d in devices]
        for d in set(devices):
            torch.cuda.synchronize(d)
        ptrs = [t.data_ptr() for t in dws]
        t1 = time.perf_counter()
        first = zkr_hip.prove_sharded_device(shards, ptrs, r, s_)     # distinct devices: proves both ways and compares (first use)
        out["first_call_ms"] = 1e3 * (time.perf_counter() - t1)
        out["first_call"] = zkr_hip.sharded_last_form()
        same = first == whole

        def timed():
            zkr_hip.prove_sharded_device(shards, ptrs, r, s_)
            t = time.perf_counter()
            for _ in range(reps):
                pr = zkr_hip.prove_sharded_device(shards, ptrs, r, s_)
            return 1e3 * (time.perf_counter() - t) / reps, pr
        ms, pr = timed()
        same = same and pr == whole
        form = zkr_hip.sharded_last_form()
        stats = zkr_hip.sharded_split_stats()
        out.update({"form": form["form"], "reason": form["reason"], "ms_per_proof": ms, "speedup_vs_whole_key": whole_ms / ms})
        if stats is not None:
            m_ = key.info()["domainSize"]
            remote = 10 * (m_ // parts) * 32 * (parts - 1) / parts     # 6 reads + 4 writes of vector-columns-of-every-block, (P - 1) / P of them remote
            out["split_phase_ms_per_shard"] = [[round(x, 4) for x in row] for row in stats]
            cross = [row[1] + row[3] for row in stats]                   # phases 2 and 4 are the cross passes (host time: enqueue -> stream idle)
            out["remote_bytes_per_shard"] = remote
            out["remote_GBps_per_shard_in_cross_phases"] = [remote / (c * 1e-3) / 1e9 if c > 0 else None for c in cross]
        os.environ["ZKR_SHARD_SPLIT_H"] = "0"
        try:
            ms0, pr0 = timed()
            out["replicated_calch_ms_per_proof"] = ms0
            out["replicated_calch_speedup_vs_whole_key"] = whole_ms / ms0
            same = same and pr0 == whole
        finally:
            del os.environ["ZKR_SHARD_SPLIT_H"]
        out["proof_identical_to_whole_key"] = bool(same)
        if not same:
            raise SystemExit("the sharded proof over devices %s differs from the whole key's proof" % devices)
    finally:
        for sh in shards:
            sh.close()
    return out


def sharding_scalars(leg):
    """The sharding leg as scalars of `config` (same keys for N = 1 and N > 1; the driver's record keeps scalars only)."""
    if not leg or "error" in leg:
        return {"sharded_error": (leg or {}).get("error")}
    if leg.get("measured"):
        return {"sharded_parts": leg["parts"], "sharded_measured": not leg["rehearsal_on_one_gpu"], "sharded_form": leg.get("form"), "sharded_reason": leg.get("reason"),
                "sharded_ms": leg.get("ms_per_proof"), "sharded_speedup": leg.get("speedup_vs_whole_key"), "sharded_replicated_calch_ms": leg.get("replicated_calch_ms_per_proof"),
                "sharded_whole_key_ms": leg["whole_key_sync_proof_ms"]}
    sp = leg.get("split_calch") or {}
    return {"sharded_parts": leg["parts"], "sharded_measured": False, "sharded_form": "projected (one GPU: shards timed one at a time, exchange modelled)",
            "sharded_ms": sp.get("projected_latency_ms", leg["projected_latency_ms_one_shard_per_gpu"]),
            "sharded_speedup": sp.get("projected_speedup", leg["projected_speedup"]), "sharded_replicated_calch_ms": leg["projected_latency_ms_one_shard_per_gpu"],
            "sharded_whole_key_ms": leg["whole_key_sync_proof_ms"], "sharded_all_on_one_gpu_ms": sp.get("all_shards_on_this_gpu_ms_per_proof"),
            "sharded_all_on_one_gpu_form": sp.get("all_shards_form")}


def verify_timed_proofs(vk_bin, proofs, pubs_of):
    """Acceptance check outside the timed region: EVERY proof goes through the native host verifier (the pairing equation of
    common.ts:30-38 / TxVerifier.sol:258-276), merged into one pairing product by a random linear combination
    (zkr_verify_batch: under 1 ms per proof).  pubs_of(i) = public signals of proof i.  Returns ms per proof."""
    import zkr_hip
    tv = time.perf_counter()
    all_pubs = [pubs_of(i) for i in range(len(proofs))]
    if not zkr_hip.verify_batch(vk_bin, proofs, all_pubs):          # one merged pairing product (zkr_verify_batch)
        for i in range(len(proofs)):                                  # locate the culprit with the single check
            if not zkr_hip.verify(vk_bin, proofs[i], all_pubs[i]):
                raise SystemExit("proof %d of the timed region does not verify" % i)
        raise SystemExit("the batch check failed although every proof verifies alone")
    return 1e3 * (time.perf_counter() - tv) / max(len(proofs), 1)


def public_signals_of(wit_tensor):
    head = wit_tensor[:32 * (N_PUBLIC + 1)].cpu().numpy().tobytes()
    return [int.from_bytes(head[32 * j:32 * j + 32], "little") for j in range(1, N_PUBLIC + 1)]


def dump_outputs(dirname, proofs):
    """--dump-outputs: the proofs of the last timed step as the caller receives them (zkr_prove's 256 bytes: pi_a (x, y) |
    pi_b (x.re, x.im, y.re, y.im) | pi_c (x, y), 32 bytes per coordinate), one byte per float32 element:
    pi_a.npy and pi_c.npy (proofs, 2, 32), pi_b.npy (proofs, 4, 32)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    b = np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(len(proofs), 8, 32).astype(np.float32)
    for name, rows in (("pi_a", slice(0, 2)), ("pi_b", slice(2, 6)), ("pi_c", slice(6, 8))):
        np.save(os.path.join(dirname, name + ".npy"), b[:, rows])


def result_head(args, value, elapsed, n_gpus, info):
    """The keys every line starts with, plain or --full: the headline figure and the workload it was measured on."""
    return {"metric": "Groth16 proofs/sec (rollup batch circuit)", "value": value, "unit": "proofs/s", "n_gpus": n_gpus,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": DTYPE, "data": "synthetic",
            "config": {"workload": "2^%d-constraint synthetic %s, 1 proof per step per GPU" % (args.log_m, "rollup circuit" if args.shape == "rollup" else "dense random R1CS"),
                       "log_m": args.log_m, "n_public": N_PUBLIC, "nVars": info["nVars"], "nnzA": info["nnzA"], "nnzB": info["nnzB"]}}


def inproc_main(args):
    """`python bench.py --gpus N --inproc`: the same measurement from ONE process without torch.distributed -- the form the
    reference's Node host takes (operator/src/snarks/common.ts:23-29 awaits its proofs from one process): the key is made on
    the first device, copied device to device to the others (zkr_key_replicate) and every step is one
    zkr_prove_batch_multi_device call of N proofs, one per GPU (proof i on device i mod N, one host thread per device
    inside the library).  --devices 0,0 (or ZKR_BENCH_ONE_GPU=1) lists the devices explicitly: the same device twice =
    two replicas side by side, the rehearsal a one-GPU box allows (never a reported scaling number)."""
    import torch
    import zkr_hip
    if args.devices:
        devices = [int(x) for x in args.devices.split(",")]
        if len(devices) != args.gpus:
            raise SystemExit("--devices lists %d devices for --gpus %d" % (len(devices), args.gpus))
    elif os.environ.get("ZKR_BENCH_ONE_GPU") == "1":
        devices = [0] * args.gpus
    else:
        devices = list(range(args.gpus))
    rehearsal = len(set(devices)) < len(devices)
    zkr_hip.synth_set_shape(1 if args.shape == "dense" else 0)
    t_setup = time.time()
    key0, w0, aux = zkr_hip.ProvingKey.synth(args.log_m, N_PUBLIC, CIRCUIT_SEED, TOXIC_SEED, device=devices[0], want_aux=args.full)
    vk_bin = key0.synth_vk(aux) if args.full else None
    del aux
    info = key0.info()
    arena_bytes = key0.arena()[1]
    keys, repl = [key0], []
    for d in devices[1:]:
        t1 = time.perf_counter()
        keys.append(key0.replicate(d, args.replicate_mode))
        dt = time.perf_counter() - t1
        repl.append({"device": d, "seconds": dt, "GBps": arena_bytes / dt / 1e9})
    n = len(devices)
    n_wit = max(1, min(4, args.steps))
    wits = []  # wits[j][i]: witness i of device slot j, resident on devices[j]
    for j, d in enumerate(devices):
        row = []
        for i in range(n_wit):
            wb = w0 if (j == 0 and i == 0) else zkr_hip.synth_witness(args.log_m, N_PUBLIC, CIRCUIT_SEED, CIRCUIT_SEED + 1000 * j + i)
            row.append(torch.frombuffer(bytearray(wb), dtype=torch.uint8).to(torch.device("cuda", d)))
        wits.append(row)
    for d in set(devices):
        torch.cuda.synchronize(d)
    setup_s = time.time() - t_setup

    def run(first, count):  # count steps of n proofs: proof index q = step * n + slot runs on keys[q mod n]
        idx = [(st, j) for st in range(first, first + count) for j in range(n)]
        return zkr_hip.prove_batch_multi_device(keys, [wits[j][st % n_wit].data_ptr() for st, j in idx],
                                                [1000003 + st * n + j for st, j in idx], [2000003 + st * n + j for st, j in idx])

    run(0, args.warmup)
    if args.full:
        keys[0].prof_enable(True)
        keys[0].prof_reset()
    sampler = GpuSampler(devices[0]).start() if args.full else None
    for d in set(devices):
        torch.cuda.synchronize(d)
    t0 = time.perf_counter()
    proofs = run(0, args.steps)
    for d in set(devices):
        torch.cuda.synchronize(d)
    elapsed = time.perf_counter() - t0
    device_state = sampler.stop() if sampler else None
    assert len(proofs) == args.steps * n
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, proofs[-n:])
    out = result_head(args, len(proofs) / elapsed, elapsed, n, info)
    out["config"].update({"parallelism": "proof-sharded x%d from ONE process (zkr_prove_batch_multi_device: one host thread per device; key copied device to device, zkr_key_replicate)%s"
                                         % (n, "; REHEARSAL: devices %s repeat one GPU" % devices if rehearsal else ""),
                          "devices": devices, "proofs_in_flight": 2})
    if not args.full:
        print(json.dumps(out))
        return
    prof = keys[0].prof()
    keys[0].prof_enable(False)
    pubs = [[public_signals_of(w) for w in row] for row in wits]
    verify_ms = verify_timed_proofs(vk_bin, proofs, lambda q: pubs[q % n][(q // n) % n_wit])
    # per device: its share of the steps over the whole region (the shares run concurrently and end together)
    roofline, whole = roofline_record(keys[0], info, prof, elapsed / args.steps, device_state, args.log_m, args.shape, devices[0])
    out.update({
        "roofline": roofline,
        "stage_ms_per_proof": {k: (v[0] / args.steps) for k, v in prof.items()},
        "key": {"arena_bytes": arena_bytes, "setup_s": setup_s, "replication": "peer-copy (zkr_key_replicate, mode %s)" % args.replicate_mode,
                "replicas": repl, "xgmi_link_GBps": 153.0},
        "proofs_verified": len(proofs), "verify_ms_per_proof_host": verify_ms,
        "device_state_during_timed_region": device_state, "hbm_whole_proof": whole,
    })
    modes = [k.replication() for k in keys[1:]]
    out["key"]["replica_modes"] = modes
    out["config"].update({"key_replication": "peer-copy: " + (",".join(sorted(set("%s%s" % (m["mode"], "" if m["peer_direct"] else " (staged through the host)") for m in modes))) or "none"),
                          "key_replicate_GBps_min": min([r_["GBps"] for r_ in repl], default=None)})
    if n > 1 and args.shards > 1:
        for k in keys[1:]:
            k.close()
        try:
            out["intra_proof_sharding"] = sharded_multi_leg(keys[0], w0, devices)
        except (Exception, SystemExit) as e:
            out["intra_proof_sharding"] = {"error": str(e)}
        out["config"].update(sharding_scalars(out["intra_proof_sharding"]))
    print(json.dumps(out))


DTYPE = "u32 limbs, 254-bit integer Montgomery (9 x 29 bits in the MSM kernels, 8 x 32 bits elsewhere)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log-m", type=int, default=20)
    ap.add_argument("--cpu-sample-log-m", type=int, default=None, help="size the CPU baseline is measured at (default: --log-m itself, capped at 2^20)")
    ap.add_argument("--shape", choices=["rollup", "dense"], default="rollup",
                    help="synthetic circuit: rollup-shaped (BASELINE configs[1..3]) or dense random (configs[4])")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--js-sample-log-m", type=int, default=12, help="size the snarkjs-shaped JS baseline is measured at (about 23 s at 2^12; scaled linearly to --log-m)")
    ap.add_argument("--no-js-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true", help="synchronous proofs, one at a time (latency)")
    ap.add_argument("--no-tx-circuit", action="store_true", help="skip the BatchProcessTx(2, 6) legs (SURVEY 8(f-3)) and the drop-in caller leg")
    ap.add_argument("--no-bcast-modes", action="store_true", help="skip timing the two key replication modes on this GPU")
    ap.add_argument("--inproc", action="store_true", help="N GPUs from ONE process through zkr_key_replicate + zkr_prove_batch_multi_device (no torch.distributed)")
    ap.add_argument("--devices", default=None, help="--inproc: comma-separated HIP ordinals, one per --gpus slot (a device may repeat)")
    ap.add_argument("--replicate-mode", choices=["auto", "full", "base"], default="auto", help="--inproc: form of the device-to-device key copy")
    ap.add_argument("--shards", type=int, default=8, help="(0 = skip) intra-proof sharding leg (SURVEY 8(e) row 2): split every MSM of ONE proof into this many contiguous point ranges, "
                                                          "run the shards one after the other on this GPU and report the per-shard time (= projected latency with one shard per GPU)")
    ap.add_argument("--no-2-22", action="store_true", help="skip the BASELINE configs[2] leg (one 2^22 key, 6 timed proofs; about 20 s)")
    ap.add_argument("--with-2-24-dense", action="store_true", help="add the BASELINE configs[4] leg (2^24 dense random R1CS: setup about 150 s)")
    ap.add_argument("--no-withdraw", action="store_true", help="skip the withdraw-circuit leg (withdraw.ts:6-10)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline figure (see the module docstring); the --no-* / --with-* / --shards options select within it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the proofs of the last timed step to DIR/pi_a.npy, pi_b.npy, pi_c.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py needs --steps >= 1 and --warmup >= 0")

    if args.inproc:
        return inproc_main(args)
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env > 1:
        # the host driver of the pool only supports dmabuf IPC: without this RCCL's first cross-process exchange fails with
        # `hipIpcGetMemHandle: invalid argument`.  Set before torch / HIP load, on EVERY launch route (the driver's own torchrun too)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus))  # plain `python bench.py --gpus N`: start the ranks as a child torchrun

    import datetime
    import torch
    import zkr_hip
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d: launch one rank per GPU (or run it plainly, it starts them itself)" % (args.gpus, world))
    # rehearsal of the N > 1 path on a one-GPU box: ZKR_BENCH_ONE_GPU=1 puts every rank on cuda:0 and
    # ZKR_BENCH_BACKEND=gloo replaces RCCL (which refuses two ranks on one device); never used for reported numbers
    one_gpu = os.environ.get("ZKR_BENCH_ONE_GPU") == "1"
    backend = os.environ.get("ZKR_BENCH_BACKEND", "nccl")
    if one_gpu:
        local = 0
    torch.cuda.set_device(local)
    dist = side = data_group = None
    if world > 1:
        import torch.distributed as dist
        # every collective is bounded: a rank that hangs in the first RCCL exchange is ended by the watchdog after this many
        # seconds and the job exits non-zero (the 4.47 GB arena takes ~30 ms per xGMI link, ~1 s through host memory)
        tmo = datetime.timedelta(seconds=int(os.environ.get("ZKR_BENCH_TIMEOUT_S", "180")))
        # The DEFAULT group is gloo (host TCP on 127.0.0.1): rendezvous, barriers, the max over ranks and the fallback agreement
        # do not depend on the GPU transport.  RCCL is a second group that only carries the key bytes; its communicator is made at
        # its first collective, i.e. inside replicate_key's try: an RCCL that cannot initialise (IPC handles refused, no peer
        # access) ends in per-rank replicas, not in a dead job.
        dist.init_process_group("gloo", timeout=tmo)
        if backend == "nccl":
            data_group = dist.new_group(backend="nccl", timeout=tmo)

    def barrier():
        if dist:
            dist.barrier(group=side)

    zkr_hip.synth_set_shape(1 if args.shape == "dense" else 0)
    # ---- key: generated on rank 0 (points computed on the GPU), replicated by one broadcast of the arena
    t_setup = time.time()
    key = None
    w0 = None
    synth = lambda want_aux: zkr_hip.ProvingKey.synth(args.log_m, N_PUBLIC, CIRCUIT_SEED, TOXIC_SEED, device=local, want_aux=want_aux)
    if rank == 0:
        key, w0, aux = synth(args.full)
        vk_bin = key.synth_vk(aux) if args.full else None  # for the native acceptance check after the timed region
        del aux
    t_bcast = time.time()
    # fallback ("replicas only"): every rank derives the key from the seeds itself -- in production: from the
    # packed key file / the provingKeyBin over its own PCIe link
    key, replication = zkr_hip.replicate_key(key, rank, world, local, lambda: synth(False)[0], dist, side, data_group=data_group)
    torch.cuda.synchronize()
    bcast_s = time.time() - t_bcast
    from zkr_hip import batch as _zb
    bcast_timing = dict(_zb.last_timing)
    info = key.info()
    arena_bytes = key.arena()[1]

    # ---- witnesses of this rank, resident in HBM before timing starts (distinct per rank and step, up to 4)
    n_wit = max(1, min(4, args.steps))
    wits = []
    for i in range(n_wit):
        wseed = CIRCUIT_SEED if (rank == 0 and i == 0) else CIRCUIT_SEED + 1000 * rank + i
        wb = w0 if (rank == 0 and i == 0) else zkr_hip.synth_witness(args.log_m, N_PUBLIC, CIRCUIT_SEED, wseed)
        wits.append(torch.frombuffer(bytearray(wb), dtype=torch.uint8).cuda(local))
    setup_s = time.time() - t_setup
    stream = torch.cuda.current_stream().cuda_stream

    # The proofs of a rollup batch are independent: they are pipelined two deep (zkr_prove_submit /
    # zkr_prove_collect), so the GPU work of proof i+1 is enqueued before the host assembles proof i.
    # --no-pipeline times fully synchronous proofs (single-proof latency).
    def run(first, count):
        if args.no_pipeline:
            return [key.prove_device(wits[i % n_wit].data_ptr(), r=1000003 + i, s=2000003 + i, stream=stream) for i in range(first, first + count)]
        idx = range(first, first + count)
        return key.prove_batch_device([wits[i % n_wit].data_ptr() for i in idx], [1000003 + i for i in idx], [2000003 + i for i in idx], stream)

    run(0, args.warmup)
    if args.full:
        key.prof_enable(True)
        key.prof_reset()
    sampler = GpuSampler(local).start() if rank == 0 and args.full else None
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    proofs = run(0, args.steps)
    torch.cuda.synchronize()
    assert len(proofs) == args.steps
    barrier()
    elapsed = time.perf_counter() - t0
    device_state = sampler.stop() if sampler else None
    per_rank = [{"rank": rank, "proofs": len(proofs), "seconds": elapsed}]
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=side)   # host tensor: gloo side group (or the gloo default group of a rehearsal)
        elapsed = float(t.item())
        parts = [None] * world
        dist.all_gather_object(parts, per_rank[0], group=side)  # outside the timed region: what every rank did, for the SCALE record
        per_rank = parts
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, proofs[-1:])
    parallelism = "proof-sharded x%d (key arena replicated once: %s)" % (world, "RCCL broadcast" if replication == "nccl" else
                                                                        replication + (", rehearsal on one GPU" if one_gpu else ""))
    if not args.full:
        if rank == 0:
            out = result_head(args, sum(p["proofs"] for p in per_rank) / elapsed, elapsed, world, info)
            out["config"].update({"parallelism": parallelism, "proofs_in_flight": 1 if args.no_pipeline else 2})
            if world > 1:
                out["per_rank"] = per_rank
            print(json.dumps(out))
        if dist:
            barrier()
            dist.destroy_process_group()
        return
    prof = key.prof()
    key.prof_enable(False)

    verified = verify_ms = None
    if rank == 0:
        pubs = [public_signals_of(w) for w in wits]
        verify_ms = verify_timed_proofs(vk_bin, proofs, lambda i: pubs[i % n_wit])
        verified = args.steps

    # The boundary as the reference's caller uses it (operator/src/snarks/common.ts:27-29: ONE proof awaited at a time, from a
    # host ArrayBuffer) -- reported in `config.boundary`, never as `value`: synchronous proofs from a resident witness
    # (latency), synchronous proofs from a pageable host witness (zkr_prove: PCIe inside the call), concurrent callers, and
    # one batch call of host buffers
    boundary = None
    if rank == 0 and world == 1:
        n_sync = 8
        key.prove_device(wits[0].data_ptr(), r=5, s=7, stream=stream)
        t1 = time.perf_counter()
        for i in range(n_sync):
            key.prove_device(wits[i % n_wit].data_ptr(), r=21 + i, s=23 + i, stream=stream)
        sync_ms = 1e3 * (time.perf_counter() - t1) / n_sync
        hw = bytes(wits[0].cpu().numpy().tobytes())
        key.prove(hw, 5, 7)
        t1 = time.perf_counter()
        for i in range(n_sync):
            key.prove(hw, 11 + i, 13 + i)
        pcie_rate = n_sync / (time.perf_counter() - t1)
        # the same boundary as concurrent callers use it (libuv workers behind Promise.all in index.js: every call
        # brings its pageable host witness; the library keeps two proofs in flight per key)
        import threading
        n_thr, per_thr = 3, 8
        ths = [threading.Thread(target=lambda j=j: [key.prove(hw, 100 + 10 * j + i, 200 + 10 * j + i) for i in range(per_thr)]) for j in range(n_thr)]
        t1 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        pcie_rate_conc = n_thr * per_thr / (time.perf_counter() - t1)
        # and as ONE caller hands over a whole batch of host buffers (zkr_prove_batch: the next witness crosses PCIe while
        # two proofs compute) -- what index.js groth16GenProofBatch / zkr_hip.prove_batch do
        hws = [bytes(w.cpu().numpy().tobytes()) for w in wits]
        n_b = 24
        key.prove_batch([hws[i % n_wit] for i in range(4)])
        t1 = time.perf_counter()
        key.prove_batch([hws[i % n_wit] for i in range(n_b)], [300 + i for i in range(n_b)], [400 + i for i in range(n_b)])
        pcie_rate_batch = n_b / (time.perf_counter() - t1)
        boundary = {"sync_latency_ms": sync_ms, "sync_resident_proofs_per_s": 1e3 / sync_ms, "host_buffer_sync_proofs_per_s": pcie_rate,
                    "host_buffer_concurrent_callers_proofs_per_s": pcie_rate_conc, "host_buffer_batch_proofs_per_s": pcie_rate_batch,
                    "note": "value = resident witnesses, two proofs in flight (zkr_prove_batch_device); the reference's caller awaits one proof at a time "
                            "from a host ArrayBuffer (common.ts:27-29): host_buffer_sync_proofs_per_s"}

    if rank == 0:
        total_proofs = sum(p["proofs"] for p in per_rank)
        assert total_proofs == args.steps * world
        value = total_proofs / elapsed
        roofline, whole = roofline_record(key, info, prof, elapsed / args.steps, device_state, args.log_m, args.shape, local)
        per_proof_ms = {k: (v[0] / args.steps) for k, v in prof.items()}
        out = result_head(args, value, elapsed, world, info)
        out["config"].update({"parallelism": parallelism,
                              "proofs_in_flight": 1 if args.no_pipeline else 2,
                              "boundary": boundary})
        out.update({
            "roofline": roofline,
            "stage_ms_per_proof": per_proof_ms,
            "per_rank": per_rank,
            "key": {"arena_bytes": arena_bytes, "setup_s": setup_s, "replication": {"nccl": "rccl"}.get(replication, replication),
                    "bcast_s": bcast_s if world > 1 else None,   # the whole replication on rank 0: collective + its synchronisation
                    "bcast_GBps": (arena_bytes / bcast_s / 1e9) if world > 1 and bcast_s > 0 and replication != "per-rank" else None,
                    # the collective alone as rank 0 saw it (receivers add the adoption of the bytes: workspace allocation, ~20 ms)
                    "bcast_wire_s": bcast_timing.get("wire_s") if world > 1 and replication != "per-rank" else None,
                    "bcast_wire_GBps": (bcast_timing["bytes"] / bcast_timing["wire_s"] / 1e9) if world > 1 and replication != "per-rank" and bcast_timing.get("wire_s") else None,
                    "xgmi_link_GBps": 153.0},  # one RCCL broadcast over xGMI: a ring / chain is bound by one link
            "pcie_inclusive_proofs_per_s": boundary and boundary["host_buffer_sync_proofs_per_s"],
            "pcie_inclusive_concurrent_callers_proofs_per_s": boundary and boundary["host_buffer_concurrent_callers_proofs_per_s"],
            "pcie_inclusive_batch_call_proofs_per_s": boundary and boundary["host_buffer_batch_proofs_per_s"],
            "proofs_verified": verified, "verify_ms_per_proof_host": verify_ms,
            "device_state_during_timed_region": device_state,
            "hbm_whole_proof": whole,
        })
        if world == 1 and not args.no_cpu_baseline:  # before the key goes: the GPU proof of the CPU leg's witness is compared with the CPU proofs
            cpu_lm = args.cpu_sample_log_m if args.cpu_sample_log_m is not None else min(args.log_m, 20)
            out["cpu_baseline"] = cpu_baseline(cpu_lm, args.log_m, gpu_key=key if args.shape == "rollup" else None)
            out["cpu_baseline"]["host_cores_available"] = effective_host_cores()
            out["cpu_baseline"]["host_hardware_threads"] = os.cpu_count()
            if not args.no_js_baseline:
                out["cpu_baseline"]["snarkjs_style"] = cpu_baseline_js(args.js_sample_log_m, args.log_m)
            cpu_baseline_scalars(out["cpu_baseline"], out["value"], args.js_sample_log_m)
        if world == 1 and not args.no_bcast_modes:
            out["key"]["replication_modes_one_gpu"] = bcast_modes_leg(key, bytes(wits[0].cpu().numpy().tobytes()), local)
        if world == 1 and args.shards > 1:
            try:
                out["intra_proof_sharding"] = shard_leg(key, wits[0], args.shards, proofs[0], local)
            except (Exception, SystemExit) as e:  # a side leg never costs the headline line; a differing proof shows here
                out["intra_proof_sharding"] = {"error": str(e)}
        elif world > 1 and args.shards > 1:
            # N > 1: ONE proof over the N devices for real (the other ranks wait at the barrier below, their GPUs idle): rank 0
            # builds shard i on device i -- no projection
            try:
                if one_gpu:
                    devs = [0] * world
                elif torch.cuda.device_count() >= world:
                    devs = list(range(world))
                else:
                    raise RuntimeError("rank 0 sees %d devices, the job has %d ranks" % (torch.cuda.device_count(), world))
                out["intra_proof_sharding"] = sharded_multi_leg(key, bytes(wits[0].cpu().numpy().tobytes()), devs)
            except (Exception, SystemExit) as e:
                out["intra_proof_sharding"] = {"error": str(e)}
        if "intra_proof_sharding" in out:
            out["config"].update(sharding_scalars(out["intra_proof_sharding"]))
        out["config"].update({"key_replication": out["key"]["replication"], "key_bcast_GBps": out["key"]["bcast_GBps"], "key_bcast_wire_GBps": out["key"]["bcast_wire_GBps"]})
        flat = out["config"]                                   # scalars next to the nested objects: what the driver's record keeps
        if boundary:
            flat.update({"sync_latency_ms": boundary["sync_latency_ms"], "sync_resident_proofs_per_s": boundary["sync_resident_proofs_per_s"],
                         "host_buffer_sync_proofs_per_s": boundary["host_buffer_sync_proofs_per_s"],
                         "host_buffer_sync_ms": 1e3 / boundary["host_buffer_sync_proofs_per_s"],
                         "host_buffer_concurrent_proofs_per_s": boundary["host_buffer_concurrent_callers_proofs_per_s"],
                         "host_buffer_batch_proofs_per_s": boundary["host_buffer_batch_proofs_per_s"]})
        side_legs = world == 1 and args.log_m == 20 and args.shape == "rollup"
        if world == 1 and (not args.no_tx_circuit or (side_legs and (not args.no_2_22 or args.with_2_24_dense or not args.no_withdraw))):
            key.close()  # its streams would share the hardware queues with the streams of the next leg's key
            key = None
        peak_gmul = (roofline.get("valu") or {}).get("peak_fq_mul_per_s_G")
        if side_legs and not args.no_2_22:                   # BASELINE configs[2]
            try:
                leg = out["config_2_22"] = size_leg(local, 22, "rollup", peak_gmul=peak_gmul, device_state=device_state)
                flat.update({"rate_2_22_proofs_per_s": leg["proofs_per_s"], "ms_per_proof_2_22": leg["ms_per_proof"], "sync_latency_ms_2_22": leg["sync_latency_ms"],
                             "proofs_verified_2_22": leg["proofs_verified"]})
                out["roofline"].update({"frac_2_22": leg["roofline"]["frac"], "achieved_2_22": leg["roofline"]["achieved"], "kernel_2_22": leg["roofline"]["kernel"],
                                        "avg_launch_ms_2_22": leg["roofline"]["avg_launch_ms"], "valu_frac_proof_2_22": leg["roofline"].get("valu_frac_proof")})
            except (Exception, SystemExit) as e:
                out["config_2_22"] = {"error": str(e)}
        if side_legs and args.with_2_24_dense:                 # BASELINE configs[4]
            try:
                leg = out["config_2_24_dense"] = size_leg(local, 24, "dense", steps=4, warmup=1, peak_gmul=peak_gmul, device_state=device_state)
                flat.update({"rate_2_24_dense_proofs_per_s": leg["proofs_per_s"], "ms_per_proof_2_24_dense": leg["ms_per_proof"],
                             "sync_latency_ms_2_24_dense": leg["sync_latency_ms"]})
                out["roofline"].update({"frac_2_24_dense": leg["roofline"]["frac"], "kernel_2_24_dense": leg["roofline"]["kernel"],
                                        "avg_launch_ms_2_24_dense": leg["roofline"]["avg_launch_ms"]})
            except (Exception, SystemExit) as e:
                out["config_2_24_dense"] = {"error": str(e)}
        if side_legs and not args.no_withdraw:
            try:
                leg = out["withdraw_circuit"] = withdraw_leg(local)
                flat.update({"withdraw_single_proof_ms": leg["single_proof_ms"], "withdraw_fused_proofs_per_s": leg["fused_proofs_per_s"],
                             "withdraw_dropin_call_ms": leg["dropin_steady_ms"], "withdraw_sequence_ms": leg["sequence_ms"]["total"]})
            except (Exception, SystemExit) as e:
                out["withdraw_circuit"] = {"error": str(e)}
        if world == 1 and not args.no_tx_circuit:
            out["dropin"] = dropin_leg(local)
            out["tx_circuit"] = tx_circuit_leg(local, max(args.steps, 4))
            # the same circuit family filled up to the headline size: 18 transactions per batch = 1 008 108 constraints, 2^20 domain
            out["rollup_circuit_2_20"] = tx_circuit_leg(local, min(max(args.steps, 4), 20), batch=18, depth=6)
            out["facade_pipeline"] = facade_pipeline_leg(local)                         # 256 batches: VERDICT r2 item 7
            out["facade_pipeline_1024"] = facade_pipeline_leg(local, n_batches=1024)  # a longer stream: the one-off builder latency weighs less
            out["facade_pipeline_host_witness"] = facade_pipeline_leg(local, chunk=32, witness="host")
            # the reference's own circuit through the drop-in boundary, kept by the driver's record with `config`
            txf = {"tx_dropin_call_ms": out["dropin"]["dropin_steady_ms"], "tx_single_proof_ms": (out["tx_circuit"]["facade_sequential"] or {}).get("proof_ms"),
                   "tx_sequence_ms": (out["tx_circuit"]["facade_sequential"] or {}).get("total_ms"),
                   "tx_fused_proofs_per_s": out["tx_circuit"]["proofs_per_s"], "tx_facade_pipeline_proofs_per_s": out["facade_pipeline_1024"]["end_to_end_proofs_per_s"],
                   "rollup_18tx_2_20_proofs_per_s": out["rollup_circuit_2_20"]["proofs_per_s"]}
            flat.update(txf)
            if out["config"]["boundary"] is not None:
                out["config"]["boundary"].update(txf)
        print(json.dumps(out))
    if dist:
        barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
