"""CPU: the audit of a finished key (zkr_key_audit, zkr_contribution_chain_check) as far as it goes without a GPU -- the equations
in the exponent against the oracle's setup (tests/key_audit_model.py), the chain check of delta records assembled from known
secrets, the refusals that come before any device call, and the code object of csrc/zkr_key_audit.hip: no scratch."""
import ctypes
import os
import re
import subprocess

import pytest

import groth16 as g
import key_audit_model as model
from test_contribution_cpu import make_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
R = g.R
D1, D2, D3 = 0x7E57AB1ED0D0CAFE, 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE, 0x1234567
TAU, ALFA, BETA, DELTA = 0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F7081, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978, 0x123456789ABCDEF0FEDCBA9876543210123456789ABCDEF, D1 * D2 % R


# ---------------------------------------------------------------- the model
def _case(m, p, power):
    circ = g.synth_circuit(m, p, 0x5A4B0001 + m)
    tox = dict(t=TAU, alfa=ALFA, beta=BETA, gamma=1, delta=DELTA)
    rng = g.SplitMix64(0xA0D17 + m)
    rho = [rng.fr() >> 126 for _ in range(circ["nVars"])]      # 128 bits
    sigma = [rng.fr() >> 126 for _ in range(m)]
    return circ, model.key_logs(circ, tox), model.transcript_logs(TAU, ALFA, BETA, 1 << power), rho, sigma


@pytest.mark.parametrize("m,p,power", [(8, 2, 3), (32, 3, 5), (8, 2, 5)], ids=["2^3", "2^5", "2^3_in_a_power_5_transcript"])
def test_the_equations_hold_in_the_exponent_for_the_oracles_setup(m, p, power):
    circ, key, tr, rho, sigma = _case(m, p, power)
    assert key["m"] == m and any(c is not None for c in key["C"]) and all(c is None for c in key["C"][:p + 1])
    assert model.equations(circ, key, tr, rho, sigma) == {e: True for e in ("E1", "E2", "E3", "E4", "E5", "E6")}


def test_each_equation_binds_what_it_names_in_the_exponent():
    """One wrong log, or one changed coefficient of the circuit, breaks the equation that speaks about it and no other."""
    circ, key, tr, rho, sigma = _case(32, 3, 5)
    n, p = key["n"], key["p"]
    all_but = lambda *bad: {e: e not in bad for e in ("E1", "E2", "E3", "E4", "E5", "E6")}

    def with_(field, i, v):
        k = dict(key)
        k[field] = list(key[field])
        k[field][i] = v
        return k
    s_priv = next(s for s in range(p + 1, n) if key["C"][s] is not None)
    assert model.equations(circ, with_("A", n // 2, (key["A"][n // 2] + 1) % R), tr, rho, sigma) == all_but("E1")
    assert model.equations(circ, with_("B", n // 3, (key["B"][n // 3] + 1) % R), tr, rho, sigma) == all_but("E2", "E3")
    assert model.equations(circ, with_("IC", 1, (key["IC"][1] + 1) % R), tr, rho, sigma) == all_but("E4")
    assert model.equations(circ, with_("C", s_priv, (key["C"][s_priv] + 1) % R), tr, rho, sigma) == all_but("E5")
    assert model.equations(circ, with_("H", 5, key["H"][6]), tr, rho, sigma) == all_but("E6")
    assert model.equations(circ, dict(key, delta=key["delta"] + 1), tr, rho, sigma) == all_but("E5", "E6")
    assert model.equations(circ, key, model.transcript_logs(TAU + 1, ALFA, BETA, 32), rho, sigma) == all_but("E1", "E2", "E3", "E4", "E5", "E6")

    def c_changed(public):
        rows = [list(r) for r in circ["rows"]]
        for c, (_, _, C) in enumerate(rows):
            for k, (s, cf) in enumerate(C):
                if (s <= p) == public and s != 0:
                    rows[c][2] = C[:k] + [(s, (cf + 1) % R)] + C[k + 1:]
                    return dict(circ, rows=[tuple(r) for r in rows])
        raise AssertionError("no such C term")
    assert model.equations(c_changed(False), key, tr, rho, sigma) == all_but("E5")      # the case zkr_r1cs_matches_key cannot see
    has_public_c = any(s <= p and s != 0 for _, _, C in circ["rows"] for s, _ in C)
    if has_public_c:
        assert model.equations(c_changed(True), key, tr, rho, sigma) == all_but("E4")


def test_the_appended_rows_and_the_transform_are_what_the_setup_used():
    """a(e_s) = iNTT(column s of polsA) evaluated at tau is A_s(tau), the log the oracle's setup gives A[s] -- for a public signal,
    whose column has its appended row, and for a private one."""
    circ, key, tr, _, _ = _case(8, 2, 3)
    polsA = g.qap_columns(circ)[0]
    for s in (0, 2, key["n"] - 1):
        e = [1 if i == s else 0 for i in range(key["n"])]
        assert model.dot(model.coefficients(polsA, e, 8), tr["tau"]) == key["A"][s]
    assert polsA[2][circ["nConstraints"] + 2] == 1


# ---------------------------------------------------------------- contribution_chain_check
def _chain():
    return [make_record(x=1, d=D1, k=11), make_record(x=D1, d=D2, k=12), make_record(x=D1 * D2 % R, d=D3, k=13)]


def _refused(records, *names):
    import zkr_hip
    assert zkr_hip.contribution_chain_check(records) is False
    msg = zkr_hip.lib().zkr_last_error().decode()
    assert "contribution chain check" in msg
    for n in names:
        assert n in msg, (n, msg)


def test_a_chain_from_the_generator_and_the_empty_chain_are_accepted():
    import zkr_hip
    recs = _chain()
    assert recs[1][:64] == recs[0][64:128] and recs[2][:64] == recs[1][64:128]
    assert zkr_hip.contribution_chain_check(recs) is True
    assert zkr_hip.contribution_chain_check(b"".join(recs)) is True
    assert zkr_hip.contribution_chain_check(recs[:1]) is True
    assert zkr_hip.contribution_chain_check([]) is True
    assert zkr_hip.contribution_chain_check(b"") is True


def test_broken_chains_are_refused_with_the_record_named():
    r0, r1, r2 = _chain()
    _refused([r1, r2], "record 0", "does not start at the generator")
    _refused([r0, r2], "record 1", "chain is broken")                                   # the middle record removed
    _refused([r0, r2, r1], "record 1", "chain is broken")                               # two records swapped
    _refused([r1, r0, r2], "record 0", "does not start at the generator")
    z = int.from_bytes(r1[320:], "little")
    _refused([r0, r1[:320] + ((z + 1) % R).to_bytes(32, "little"), r2], "record 1", "knowledge of d")
    _refused([r0[:320] + (5).to_bytes(32, "little")], "record 0", "knowledge of d")


def test_chain_check_null_arguments():
    import zkr_hip
    L = zkr_hip.lib()
    ok = ctypes.c_int(7)
    assert L.zkr_contribution_chain_check(None, 1, ctypes.byref(ok)) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_contribution_chain_check(bytes(352), 1, None) == -5
    assert L.zkr_contribution_chain_check(None, 0, ctypes.byref(ok)) == 0 and ok.value == 1


# ---------------------------------------------------------------- zkr_key_audit: what is refused before any device call
def _vk(n_ic):
    return bytes(448) + n_ic.to_bytes(4, "little") + bytes(64 * n_ic)


def _audit(key, cs, ptau, vk, ok, rep=None, ptau_len=None, vk_len=None):
    import zkr_hip
    L = zkr_hip.lib()
    return L.zkr_key_audit(key, cs, ptau, len(ptau) if ptau_len is None else ptau_len, None, 0, None, 0, vk, len(vk) if vk_len is None else vk_len, ok, rep)


def test_audit_null_pointers_are_argument_errors():
    import zkr_hip
    L = zkr_hip.lib()
    t, vk = zkr_hip.ptau_new(2), _vk(3)
    ok = ctypes.c_int(7)
    rep = (ctypes.c_uint64 * 4)()
    assert _audit(None, None, t, vk, ctypes.byref(ok), rep) == -5 and b"null" in L.zkr_last_error()      # a good transcript and vk: the handles are missed
    assert ok.value == 0
    assert L.zkr_key_audit(None, None, None, 0, None, 0, None, 0, vk, len(vk), ctypes.byref(ok), rep) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_key_audit(None, None, t, len(t), None, 0, None, 0, None, 0, ctypes.byref(ok), rep) == -5 and b"null" in L.zkr_last_error()
    assert _audit(None, None, t, vk, None, rep) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_key_audit(None, None, t, len(t), None, 1, None, 0, vk, len(vk), ctypes.byref(ok), rep) == -5 and b"null" in L.zkr_last_error()   # records announced, none given
    assert L.zkr_key_audit(None, None, t, len(t), None, 0, None, 2, vk, len(vk), ctypes.byref(ok), rep) == -5 and b"null" in L.zkr_last_error()


@pytest.mark.parametrize("what,needle", [("truncated", b"length"), ("magic", b"magic"), ("shorter than a header", b"header"), ("vk_len off by one", b"IC count"),
                                         ("vk_len one short", b"IC count"), ("vk shorter than its fixed part", b"IC count")])
def test_malformed_transcripts_and_vk_lengths_are_refused_before_the_key_is_looked_at(what, needle):
    """With a null key handle: the refusal names the transcript or the verifying key, so it came before the handle was missed --
    and long before any device call (this test runs without a GPU)."""
    import zkr_hip
    L = zkr_hip.lib()
    t, vk = zkr_hip.ptau_new(2), _vk(3)
    ok = ctypes.c_int(7)
    args = {"truncated": dict(ptau=t[:-1]), "magic": dict(ptau=b"ZKRPTAU0" + t[8:]), "shorter than a header": dict(ptau=t[:16]), "vk_len off by one": dict(vk=vk + b"\0"),
            "vk_len one short": dict(vk=vk[:-1]), "vk shorter than its fixed part": dict(vk=vk[:300])}[what]
    assert _audit(None, None, args.get("ptau", t), args.get("vk", vk), ctypes.byref(ok)) == -5
    msg = L.zkr_last_error()
    assert needle in msg and b"null" not in msg, msg
    assert ok.value == 0


def test_python_host_exposes_the_audit():
    import zkr_hip
    assert zkr_hip.KeyAudit._fields == ("valid", "step", "detail", "phase1_contributions", "delta_contributions")
    assert callable(zkr_hip.ProvingKey.audit) and callable(zkr_hip.contribution_chain_check)


# ---------------------------------------------------------------- the code object
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_key_audit_kernels_use_no_scratch(tmp_path):
    """The compiler's own metadata, read as tests/test_ptau_cpu.py reads it: no kernel of zkr_key_audit.hip keeps a stack frame, and
    the kernels the unit adds are there."""
    out = tmp_path / "zkr_key_audit.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
                           "--cuda-device-only", "-S", os.path.join(ROOT, "simple-zk-rollups_amd", "csrc", "zkr_key_audit.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    rows = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        rows[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2)).group(1))
    for kernel in ("audit_scalars_kernel", "audit_c_rows_kernel", "audit_c_rows_wide_kernel", "spmv_kernel", "spmv_wide_kernel", "bitrev_copy_kernel"):
        assert any(kernel in k for k in rows), kernel
    assert {k: v for k, v in rows.items() if v} == {}
