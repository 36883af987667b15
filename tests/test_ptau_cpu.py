"""CPU: the host side of the powers-of-tau transcript (zkr_ptau_new, zkr_ptau_record_check) against records assembled here from
known secrets with the oracle's point arithmetic (oracle/bn254.py) and the library's host MiMC sponge, the way
tests/test_contribution_cpu.py builds the delta record; the argument checks of the entry points; the forgery that makes the
transcript necessary, as an executable statement (oracle only); and the code object of csrc/zkr_ptau.hip: no scratch."""
import ctypes
import os
import re
import subprocess

import pytest

from test_contribution_cpu import g1b, g2b, le, twist_point_outside_g2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

TAU1, ALFA1, BETA1 = 0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F7081, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978, 0x123456789ABCDEF0FEDCBA9876543210123456789ABCDEF
TAU2, ALFA2, BETA2 = 0x2468ACE013579BDF02468ACE13579BDF2468ACE013579BDF0246, 0x1F2E3D4C5B6A79880112233445566778899AABBCCDDEEFF, 0x0CAFEBABEDEADBEEF0123456789ABCDEFFEDCBA9876543210CAFE
NONCES = (0x0BADC0FFEE0DDF00D5EED, 0x5EC0DD0123456789, 0x7411D0FF1CE)
# record offsets: before / after of tau, alfa, beta; the two G2 images; the three R; the three z
O_BEFORE, O_AFTER, O_TAU2, O_BETA2, O_R, O_Z = (0, 128, 256), (64, 192, 320), 384, 512, (640, 704, 768), (832, 864, 896)


def make_record(before=(1, 1, 1), secrets=(TAU1, ALFA1, BETA1), nonces=NONCES, tau_for_g2=None, with_tag=True):
    """before: the discrete logs of tau1, alfa1, beta1 before the contribution.  Each proof: R = k before, c = H(tag, before, after,
    [G2 image], R), z = k + c s."""
    import bn254 as b
    from zkr_hip import rollup as n
    bef = [b.g1_mul(b.G1_GEN, x) for x in before]
    aft = [b.g1_mul(p, s) for p, s in zip(bef, secrets)]
    tau2 = b.g2_mul(b.G2_GEN, before[0] * (secrets[0] if tau_for_g2 is None else tau_for_g2) % b.R)
    beta2 = b.g2_mul(b.G2_GEN, before[2] * secrets[2] % b.R)
    rs = [b.g1_mul(p, k) for p, k in zip(bef, nonces)]
    zs = []
    for i in range(3):
        words = ([i + 1] if with_tag else []) + [bef[i][0], bef[i][1], aft[i][0], aft[i][1]]
        if i != 1:
            g2 = tau2 if i == 0 else beta2
            words += [g2[0][0], g2[0][1], g2[1][0], g2[1][1]]
        words += [rs[i][0], rs[i][1]]
        zs.append((nonces[i] + n.multi_hash(words) * secrets[i]) % b.R)
    return (b"".join(g1b(bef[i]) + g1b(aft[i]) for i in range(3)) + g2b(tau2) + g2b(beta2) + b"".join(g1b(p) for p in rs) + b"".join(le(z) for z in zs))


def _put(rec, off, piece):
    return rec[:off] + piece + rec[off + len(piece):]


def _refused(records, *names):
    import zkr_hip
    assert zkr_hip.ptau_record_check(records) is False
    msg = zkr_hip.lib().zkr_last_error().decode()
    assert "ptau record check" in msg
    for n in names:
        assert n in msg, (n, msg)


@pytest.mark.parametrize("K", [1, 3])
def test_new_transcript_is_all_generators(K):
    import bn254 as b
    import zkr_hip
    t = zkr_hip.ptau_new(K)
    M = 1 << K
    assert len(t) == 160 + 384 * M
    assert t[:32] == b"ZKRPTAU1" + K.to_bytes(4, "little") + bytes(4) + len(t).to_bytes(8, "little") + bytes(8)
    assert t[32:] == g1b(b.G1_GEN) * (2 * M) + g2b(b.G2_GEN) * M + g1b(b.G1_GEN) * (2 * M) + g2b(b.G2_GEN)


def test_records_from_known_secrets_pass_alone_and_chained():
    import bn254 as b
    import zkr_hip
    r1 = make_record()
    assert len(r1) == zkr_hip.PTAU_RECORD_BYTES == 928
    assert zkr_hip.ptau_record_check(r1) is True
    r2 = make_record(before=(TAU1, ALFA1, BETA1), secrets=(TAU2, ALFA2, BETA2), nonces=(11, 12, 13))
    assert r2[O_BEFORE[0]:O_BEFORE[0] + 64] == r1[O_AFTER[0]:O_AFTER[0] + 64]
    assert zkr_hip.ptau_record_check([r1, r2]) is True
    assert zkr_hip.ptau_record_check(r1 + r2) is True
    assert r2[O_TAU2:O_TAU2 + 128] == g2b(b.g2_mul(b.G2_GEN, TAU1 * TAU2 % b.R))
    assert zkr_hip.ptau_record_check(b"") is True   # no contribution yet: nothing to refuse


def test_each_single_fault_of_a_record_is_refused_and_named():
    import bn254 as b
    r1 = make_record()
    r2 = make_record(before=(TAU1, ALFA1, BETA1), secrets=(TAU2, ALFA2, BETA2), nonces=(11, 12, 13))
    z_alfa = int.from_bytes(r1[O_Z[1]:O_Z[1] + 32], "little")
    _refused(_put(r1, O_Z[1], le((z_alfa + 1) % b.R)), "record 0", "knowledge of alfa")
    _refused(r2 + r1, "record 0", "does not start at the generator")
    _refused(r1 + r1, "record 1", "chain is broken")
    _refused([r1, _put(r2, O_Z[2], le(5))], "record 1", "knowledge of beta")
    _refused(make_record(tau_for_g2=TAU1 + 1), "record 0", "tau1_after and tau2_after")
    _refused(_put(r1, O_AFTER[2], r1[O_BEFORE[2]:O_BEFORE[2] + 64]), "beta did not move")
    _refused(make_record(secrets=(TAU1, 1, BETA1)), "alfa did not move")
    x = int.from_bytes(r1[O_AFTER[0]:O_AFTER[0] + 32], "little")
    assert x + b.Q < 1 << 256
    _refused(_put(r1, O_AFTER[0], le(x + b.Q)), "tau proof", "out of range")
    y = int.from_bytes(r1[O_R[1] + 32:O_R[1] + 64], "little")
    _refused(_put(r1, O_R[1] + 32, le((y + 1) % b.Q)), "alfa proof", "off the curve")
    _refused(_put(r1, O_BETA2, g2b(twist_point_outside_g2())), "beta2_after is not a member of G2")
    _refused(_put(r1, O_TAU2, bytes(128)), "tau2_after is not a member of G2")
    z = int.from_bytes(r1[O_Z[0]:O_Z[0] + 32], "little")
    _refused(_put(r1, O_Z[0], le(z + b.R)), "z_tau is not below r")
    _refused(make_record(with_tag=False), "record 0", "knowledge of tau")   # the challenge without its domain tag


def test_argument_checks():
    import zkr_hip
    L = zkr_hip.lib()
    out, n, ok = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
    rec = ctypes.create_string_buffer(928)
    t = zkr_hip.ptau_new(1)
    assert L.zkr_ptau_new(3, None, ctypes.byref(n)) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_ptau_new(3, ctypes.byref(out), None) == -5
    for power in (0, 25):
        assert L.zkr_ptau_new(power, ctypes.byref(out), ctypes.byref(n)) == -5
        assert b"power" in L.zkr_last_error()
    assert L.zkr_ptau_record_check(None, 1, ctypes.byref(ok)) == -5
    assert L.zkr_ptau_record_check(bytes(928), 1, None) == -5
    assert L.zkr_ptau_contribute(None, 0, None, 0, ctypes.byref(out), ctypes.byref(n), ctypes.cast(rec, ctypes.c_char_p)) == -5
    assert L.zkr_ptau_contribute(t, len(t), None, 0, None, ctypes.byref(n), ctypes.cast(rec, ctypes.c_char_p)) == -5
    assert L.zkr_ptau_contribute(t, len(t), None, 0, ctypes.byref(out), ctypes.byref(n), None) == -5
    assert L.zkr_ptau_verify(None, 0, None, 0, 0, ctypes.byref(ok), None) == -5
    assert L.zkr_ptau_verify(t, len(t), None, 0, 0, None, None) == -5
    assert L.zkr_ptau_verify(t, len(t), None, 1, 0, ctypes.byref(ok), None) == -5     # records announced, none given
    assert L.zkr_setup_r1cs_ptau(None, 0, t, len(t), 0, ctypes.byref(out), ctypes.byref(out), ctypes.byref(n)) == -5
    assert L.zkr_setup_r1cs_ptau(bytes(12), 12, None, 0, 0, ctypes.byref(out), ctypes.byref(out), ctypes.byref(n)) == -5
    assert L.zkr_points_scale_each(None, bytes(32), 1, 0, 0) == -5
    assert L.zkr_points_scale_each(bytes(64), None, 1, 0, 0) == -5
    assert L.zkr_group_ntt(None, 3, 0, 0, 0) == -5
    buf = ctypes.create_string_buffer(128)
    assert L.zkr_group_ntt(buf, 0, 0, 0, 0) == -5 and L.zkr_group_ntt(buf, 26, 0, 0, 0) == -5
    # a transcript whose header and length disagree is an argument error wherever it is passed
    for bad in (t[:-1], b"ZKRPTAU0" + t[8:], t[:8] + (2).to_bytes(4, "little") + t[12:]):
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.ptau_contribute(bad, (TAU1, ALFA1, BETA1))
        assert e.value.code == -5


def test_no_device_means_loud_failure_not_fallback():
    import zkr_hip
    if zkr_hip.device_count() > 0:
        pytest.skip("a HIP device is present")
    r1cs = zkr_hip.binarify_r1cs(dict(nVars=3, nPubInputs=0, nOutputs=1, constraints=[[{"1": "1"}, {"2": "1"}, {"1": "1"}]]))   # domain 4
    calls = [lambda: zkr_hip.ptau_contribute(zkr_hip.ptau_new(1), (TAU1, ALFA1, BETA1)),
             lambda: zkr_hip.ptau_verify(zkr_hip.ptau_new(1)),
             lambda: zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, zkr_hip.ptau_new(2)),
             lambda: zkr_hip.group_ntt(bytes(128)),
             lambda: zkr_hip.points_scale_each(bytes(64), le(3))]
    for call in calls:
        with pytest.raises(zkr_hip.ZkrError) as e:
            call()
        assert e.value.code == -1 and "no CPU fallback" in str(e.value)


def test_a_one_party_setup_is_forgeable_whatever_happens_to_delta_afterwards():
    """Why the transcript exists.  Party 1 ran the setup and knows t, alfa, beta; a later contributor re-randomised delta with a d
    party 1 never sees.  Party 1 still proves FALSE statements: the key publishes hExps[0] = Z(t) / delta' G1, party 1 knows Z(t),
    so it holds (1 / delta') G1 and can solve the verification equation for C with A, B and the public signals of its choice."""
    import bn254 as b
    import groth16 as g
    circ = g.synth_circuit(16, 3, 0x5A4B0001)
    tox = g.toxic_from_seed(0x5A4B00FF)
    d = 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE
    pk, vk = g.setup(circ, dict(tox, delta=tox["delta"] * d % g.R))         # the contributed key: delta' = delta d
    # --- the forger: t, alfa, beta, gamma of its own setup and the PUBLISHED key; neither d nor delta'
    t, alfa, beta = tox["t"], tox["alfa"], tox["beta"]
    m = pk["domainSize"]
    z_t = (pow(t, m, g.R) - 1) % g.R
    inv_delta_g1 = b.g1_mul(pk["hExps"][0], b.inv(z_t, g.R))                # (1 / delta') G1
    sc = g.setup_scalars(circ, dict(tox, delta=1))                          # a_s(t), b_s(t), c_s(t): no delta in them
    public = [5, 6, 7]                                                      # made up: no witness has these outputs
    w_pub = [1] + public
    kx = sum(w * (beta * sc["a"][i] + alfa * sc["b"][i] + sc["c"][i]) for i, w in enumerate(w_pub)) % g.R
    a, bb = 0x1234567, 0x89ABCDEF
    proof = dict(pi_a=b.g1_mul(b.G1_GEN, a), pi_b=b.g2_mul(b.G2_GEN, bb), pi_c=b.g1_mul(inv_delta_g1, (a * bb - alfa * beta - kx) % g.R))
    assert g.is_valid(vk, proof, public) is True
    assert g.is_valid(vk, proof, [5, 6, 8]) is False                        # the forgery is for the statement it chose


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ptau_kernels_use_no_scratch(tmp_path):
    """The compiler's own metadata: no kernel of zkr_ptau.hip keeps a stack frame (a run-time indexed per-thread digit table or a
    point copied through a local would show here), and the instances the transcript needs exist for both groups."""
    out = tmp_path / "zkr_ptau.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
                           "--cuda-device-only", "-S", os.path.join(ROOT, "simple-zk-rollups_amd", "csrc", "zkr_ptau.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    rows = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        rows[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2)).group(1))
    for kernel in ("group_scale_each_kernel", "group_butterfly_kernel", "group_bitrev_kernel", "group_on_curve_kernel"):
        inst = [k for k in rows if kernel in k]
        assert len(inst) == 2 and any("G2C" in k or "Fq2" in k for k in inst), (kernel, inst)   # G1 and G2
    for kernel in ("group_combine_kernel",):
        inst = [k for k in rows if kernel in k]
        assert len(inst) == 2 and any("G2C" in k for k in inst), (kernel, inst)
    assert [k for k in rows if "group_order_check_kernel" in k and "G2C" in k] and [k for k in rows if "group_diff_kernel" in k and "G1C" in k]
    for kernel in ("fr_to_std_kernel", "twiddle_table_kernel", "ptau_coords_in_kernel", "ptau_coords_out_kernel"):
        assert any(kernel in k for k in rows), kernel
    assert {k: v for k, v in rows.items() if v} == {}
