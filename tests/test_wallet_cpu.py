"""CPU: the programs the wallet kernels run per item (csrc/wallet_program.hpp: format_privkey, pubkey, sign, the withdraw witness),
run on the host through their test hooks, against the host calls they stand in for and against oracle/rollup.py; the argument
checks of the batch calls, which come before any device is looked at; and the kernels' resources from the compiler's metadata."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import rollup as o
import wallet_cases as wc
import zkr_hip
from zkr_hip import rollup as n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
R = o.R


def _le(v):
    return int(v).to_bytes(32, "little")


def test_case_list_holds_every_text_length_and_the_reference_pairs():
    keys = wc.keys()
    assert len(keys) == wc.N_KEYS and keys[:3] == (0, 1, R - 1)
    lens = [wc.text_len(k) for k in keys]
    assert 64 in lens and 63 in lens and min(lens) <= 62
    got = wc.by_text_length()
    assert wc.text_len(got[64]) == 64 and wc.text_len(got[63]) == 63 and wc.text_len(got[62]) <= 62
    for priv, pub in wc.kat_pairs():
        assert priv in keys and n.gen_public_key(priv) == pub


def test_format_and_pubkey_programs_equal_the_host_calls_and_the_oracle():
    for k, of, op in zip(wc.keys(), wc.oracle_formatted(), wc.oracle_pubs()):
        f, pub = n.wallet_pubkey_program_host(k)
        assert f == n.format_priv_key(k) == of, k
        assert pub == n.gen_public_key(k) == op, k


@pytest.mark.parametrize("arity", [1, 5, 8])
def test_sign_program_equals_the_host_call_and_the_oracle(arity):
    for k, m, pub in zip(wc.keys(), wc.messages(arity), wc.oracle_pubs()):
        sig = n.wallet_sign_program_host(k, m)
        assert sig == n.sign(k, m), (k, arity)
        assert (sig["R8"][0], sig["R8"][1], sig["S"]) == tuple(o.sign(k, list(m))), (k, arity)
        assert n.verify(m, sig, pub)


def test_withdraw_program_equals_the_host_builder_byte_for_byte():
    c = n.WithdrawCircuit()
    assert c.n_vars * 32 == len(c.calculate_witness({"privateKey": 1, "nullifier": 2}))
    for f, nul, pub in zip(wc.oracle_formatted(), wc.nullifiers(), wc.oracle_pubs()):
        for nu in (nul, 0, R - 1):
            case = {"privateKey": f, "nullifier": nu}
            w, stmt = c.witness_program_host(case)
            assert stmt is None and w == c.calculate_witness(case), (f, nu)
            assert tuple(c.public_signals(w)) == (pub[0], pub[1], nu)


def test_withdraw_program_refuses_a_key_past_253_bits():
    c = n.WithdrawCircuit()
    w, stmt = c.witness_program_host({"privateKey": 1 << 253, "nullifier": 5})
    assert w is None and stmt == "private key fits 253 bits"
    with pytest.raises(zkr_hip.ZkrError) as e:
        c.calculate_witness({"privateKey": 1 << 253, "nullifier": 5})
    assert e.value.code == -7 and stmt in str(e.value)
    w, stmt = c.witness_program_host({"privateKey": (1 << 253) - 1, "nullifier": 5})
    assert stmt is None and w == c.calculate_witness({"privateKey": (1 << 253) - 1, "nullifier": 5})
    out, st = ctypes.create_string_buffer(c.n_vars * 32), ctypes.c_uint32()
    assert zkr_hip.lib().zkr_withdraw_witness_program_host(_le(1), _le(R), out, ctypes.byref(st)) == -5


def _refused(call, word):
    with pytest.raises(zkr_hip.ZkrError) as e:
        call()
    assert e.value.code == -5 and word in str(e.value), str(e.value)


def test_batch_calls_check_their_arguments_before_the_device():
    """Code -5 with the item's index in the message, with or without a GPU: the checks come first."""
    rng = random.Random(7)
    keys = [rng.randrange(R) for _ in range(70)]
    bad = list(keys)
    bad[37] = R
    bad[50] = R + 1
    for call in (n.format_priv_key_batch, n.gen_public_key_batch):
        _refused(lambda: call(bad), "item 37")
    msgs = [[rng.randrange(R) for _ in range(5)] for _ in keys]
    _refused(lambda: n.sign_batch(bad, msgs), "item 37")
    badm = [list(m) for m in msgs]
    badm[12][3] = R
    _refused(lambda: n.sign_batch(keys, badm), "item 12")
    L = zkr_hip.lib()
    kb, mb = b"".join(_le(k) for k in keys), b"".join(_le(v) for m in msgs for v in m)
    out = ctypes.create_string_buffer(96 * 70)
    assert L.zkr_babyjub_format_privkey_batch(None, 70, out, 0) == -5 and L.zkr_babyjub_format_privkey_batch(kb, 70, None, 0) == -5
    assert L.zkr_babyjub_pubkey_batch(None, 70, out, 0) == -5 and L.zkr_babyjub_pubkey_batch(kb, 70, None, 0) == -5
    assert L.zkr_eddsa_sign_batch(None, mb, 5, 70, out, 0) == -5 and L.zkr_eddsa_sign_batch(kb, None, 5, 70, out, 0) == -5
    assert L.zkr_eddsa_sign_batch(kb, mb, 5, 70, None, 0) == -5 and b"null" in L.zkr_last_error()
    for arity in (0, 65):
        assert L.zkr_eddsa_sign_batch(kb, mb, arity, 1, out, 0) == -5 and b"arity" in L.zkr_last_error()
    assert out.raw == bytes(96 * 70)   # outputs untouched
    # the withdraw witnesses: null pointers, a key = r, a nullifier = r (the pointer is never followed: the checks come first)
    dummy = ctypes.c_void_p(64)
    assert L.zkr_withdraw_witness_batch_device(None, kb, 70, dummy, 0, None) == -5
    assert L.zkr_withdraw_witness_batch_device(kb, None, 70, dummy, 0, None) == -5
    assert L.zkr_withdraw_witness_batch_device(kb, kb, 70, None, 0, None) == -5
    badb = b"".join(_le(k) for k in bad)
    assert L.zkr_withdraw_witness_batch_device(badb, kb, 70, dummy, 0, None) == -5 and b"witness 37" in L.zkr_last_error()
    assert L.zkr_withdraw_witness_batch_device(kb, badb, 70, dummy, 0, None) == -5 and b"witness 37" in L.zkr_last_error()
    for hook in (lambda: n.wallet_pubkey_program_host(R), lambda: n.wallet_sign_program_host(R, [1]), lambda: n.wallet_sign_program_host(1, [R])):
        _refused(hook, ">= r")


def test_empty_batches_are_empty_results():
    assert n.format_priv_key_batch([]) == [] and n.gen_public_key_batch([]) == [] and n.sign_batch([], []) == []
    L = zkr_hip.lib()
    assert L.zkr_babyjub_format_privkey_batch(None, 0, None, 0) == 0 and L.zkr_babyjub_pubkey_batch(None, 0, None, 0) == 0
    assert L.zkr_eddsa_sign_batch(None, None, 5, 0, None, 0) == 0 and L.zkr_withdraw_witness_batch_device(None, None, 0, None, 0, None) == 0
    with pytest.raises(ValueError):
        n.sign_batch([1, 2], [[1]])
    with pytest.raises(ValueError):
        n.sign_batch([1, 2], [[1], [1, 2]])


def test_no_gpu_means_no_device_not_a_host_fallback():
    if zkr_hip.device_count() > 0:
        pytest.skip("a HIP device is present")
    keys = list(wc.keys()[:3])
    for call in (lambda: n.format_priv_key_batch(keys), lambda: n.gen_public_key_batch(keys), lambda: n.sign_batch(keys, [[1, 2]] * 3)):
        with pytest.raises(zkr_hip.ZkrError) as e:
            call()
        assert e.value.code == -1 and "no CPU fallback" in str(e.value)
    kb = b"".join(_le(1) for _ in range(3))
    assert zkr_hip.lib().zkr_withdraw_witness_batch_device(kb, kb, 3, ctypes.c_void_p(64), 0, None) == -1


def test_wallet_kernels_use_no_scratch(tmp_path):
    """The compiler's own metadata, read as tools/kernel_resources.py reads it: no kernel of zkr_wallet.hip spills or keeps a stack
    frame -- the programs take their scalars' bits from shifting registers and are inlined whole."""
    out = tmp_path / "zkr_wallet.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
                           "--cuda-device-only", "-S", os.path.join(ROOT, "simple-zk-rollups_amd", "csrc", "zkr_wallet.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    rows = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        g = lambda key: int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", m.group(2)).group(1))
        rows[m.group(1)] = (g("private_segment_fixed_size"), g("next_free_vgpr"))
    for name in ("wallet_format_kernel", "wallet_pubkey_kernel", "wallet_sign_kernel", "withdraw_witness_kernel", "withdraw_layout_kernel"):
        assert len([k for k in rows if name in k]) == 1, name
    assert {k: v for k, v in rows.items() if v[0]} == {}
    assert max(v[1] for v in rows.values()) <= 512   # __launch_bounds__(64): one wavefront's whole register file at the most
