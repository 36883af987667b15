"""CPU: the host side of the evaluation-form side tables derived from a key's own points (include/zkr.h zkr_key_eval_tables,
csrc/zkr_eval_tables.hip): the argument checks that need no device, the four symbols in the header, the library and the binding, the
code object of the per-slot addition (no scratch, both groups), and a model of the three formulas the derivation rests on

    E'_j = ke 1/m sum_i (g w^j)^(-i) H_i        ke = -1/2 R / m^2
    F_j  =    1/m sum_i w^(-ij) H_i
    C'_s = C_s + 1/2 sum_j C_js F_j

as naive sums over the POINTS of an oracle setup (oracle/groth16.py, oracle/bn254.py) at m = 8, against scalar x generator for the
scalars csrc/eval_h.hpp makes from the same setup's toxic values (through the host shim).  The model is a specification: it holds
whether or not the derivation exists."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import bn254 as b
import groth16 as g
from test_eval_h_cpu import _builder, _circuit

R = g.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simple-zk-rollups_amd", "csrc")
SHIM = os.environ.get("ZKR_HOSTARITH_LIB") or os.path.join(CSRC, "libzkr_hostarith.so")
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("zkr_key_eval_tables", "zkr_key_eval_tables_drop", "zkr_key_eval_tables_equal", "zkr_points_add_each")


def _r1cs():
    import zkr_hip
    return zkr_hip.binarify_r1cs(dict(nVars=3, nPubInputs=0, nOutputs=1, constraints=[[{"1": "1"}, {"2": "1"}, {"1": "1"}]]))   # domain 4


def test_argument_checks_need_no_device():
    """Null pointers, unknown flags and a malformed system are refused before anything looks at the key or at a device: the key
    here is a buffer of zeros that must never be read."""
    import zkr_hip
    L = zkr_hip.lib()
    key = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    built, same = ctypes.c_int(7), ctypes.c_int(7)
    r1cs = _r1cs()
    assert L.zkr_key_eval_tables(None, r1cs, len(r1cs), 0, ctypes.byref(built)) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_key_eval_tables(key, None, 0, 0, ctypes.byref(built)) == -5
    assert L.zkr_key_eval_tables(key, r1cs, len(r1cs), 0, None) == -5
    assert L.zkr_key_eval_tables(key, r1cs, len(r1cs), 1, ctypes.byref(built)) == -5 and b"flags" in L.zkr_last_error()
    three = (3).to_bytes(4, "little")
    for bad, what in ((r1cs[:-1], b"truncated"), (r1cs + b"\0", b"trailing"), (r1cs[:8], b"header"),
                      (r1cs[:4] + three + r1cs[8:], b"geometry"),          # nPublic = nVars
                      (r1cs[:16] + three + r1cs[20:], b"out of range")):   # the first term of A names signal 3 of 3
        built.value = 7
        assert L.zkr_key_eval_tables(key, bad, len(bad), 0, ctypes.byref(built)) == -5, what
        assert what in L.zkr_last_error(), (what, L.zkr_last_error())
        assert built.value == 0
    assert L.zkr_key_eval_tables_drop(None) == -5
    assert L.zkr_key_eval_tables_equal(None, key, ctypes.byref(same)) == -5 and L.zkr_key_eval_tables_equal(key, None, ctypes.byref(same)) == -5
    assert L.zkr_key_eval_tables_equal(key, key, None) == -5
    assert L.zkr_points_add_each(None, bytes(64), 1, 0, 0) == -5 and L.zkr_points_add_each(bytes(64), None, 1, 0, 0) == -5


def test_no_device_means_loud_failure_not_fallback():
    import zkr_hip
    if zkr_hip.device_count() > 0:
        pytest.skip("a HIP device is present")
    L = zkr_hip.lib()
    key = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)   # never read: there is no device a key could be on
    built = ctypes.c_int(7)
    r1cs = _r1cs()
    assert L.zkr_key_eval_tables(key, r1cs, len(r1cs), 0, ctypes.byref(built)) == -1 and b"no CPU fallback" in L.zkr_last_error()
    assert built.value == 0
    for g2 in (False, True):
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.points_add_each(bytes(128 if g2 else 64), bytes(128 if g2 else 64), g2=g2)
        assert e.value.code == -1 and "no CPU fallback" in str(e.value)


def test_the_four_symbols_are_in_the_header_the_library_and_the_binding():
    import zkr_hip
    header = open(os.path.join(ROOT, "include", "zkr.h")).read()
    L = zkr_hip.lib()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        fn = getattr(L, name)          # AttributeError when the library lacks it
        assert fn.argtypes, name       # ... and the binding declared its arguments
    for method in ("eval_tables", "drop_eval_tables", "eval_tables_equal"):
        assert callable(getattr(zkr_hip.ProvingKey, method))
    assert callable(zkr_hip.points_add_each)
    with pytest.raises(ValueError):
        zkr_hip.points_add_each(bytes(64), bytes(128))


def _bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2)


def test_model_of_the_three_formulas_over_points():
    """m = 8.  The key holds H bit-reversed (slot j = power bitrev(j)) and C above nPublic; everything below is sums of those points."""
    shim = ctypes.CDLL(SHIM)
    rng = random.Random(0x5A4B0E7)
    logm, p = 3, 2
    m = 1 << logm
    circ, _ = _circuit(m, p, rng, True, True)
    n = circ["nVars"]
    tox = dict(t=rng.randrange(2, R), alfa=rng.randrange(1, R), beta=rng.randrange(1, R), gamma=rng.randrange(1, R), delta=rng.randrange(1, R))
    sc = g.setup_scalars(circ, tox)
    pk, _ = g.setup(circ, tox)
    hx = [x % R for x in sc["h"][:m]]
    cpriv = [sc["cpriv"][s] % R for s in range(p + 1, n)]
    _, _, cfold, eprime = _builder(shim, hx, logm, circ, cpriv)       # what the scalar-knowing setup multiplies the generator by

    slots = [pk["hExps"][_bitrev(j, logm)] for j in range(m)]          # the key's H table
    H = [None] * m
    for j in range(m):
        H[_bitrev(j, logm)] = slots[j]                                 # power order again
    assert H == pk["hExps"][:m]

    def comb(points, scalars):
        acc = None
        for P, k in zip(points, scalars):
            acc = b.g1_add(acc, b.g1_mul(P, k % R))
        return acc

    w, gcos = g.root_of_unity(m), g.root_of_unity(2 * m)
    minv, half = b.inv(m, R), b.inv(2, R)
    ke = -half * pow(2, 256, R) * minv * minv % R
    for j in range(m):
        x = b.inv(gcos * pow(w, j, R) % R, R)
        assert comb(H, [ke * minv * pow(x, i, R) for i in range(m)]) == b.g1_mul(b.G1_GEN, eprime[j]), j
    F = [comb(H, [minv * pow(w, -i * j % m, R) for i in range(m)]) for j in range(m)]
    public_with_a_point = 0
    for s in range(n):
        col = sc["polsC"][s]
        fold = comb([F[j] for j in col], [half * cf for cf in col.values()])
        own = pk["C"][s] if s > p else None                            # C_s = infinity for the public signals
        assert b.g1_add(own, fold) == b.g1_mul(b.G1_GEN, cfold[s]), s
        public_with_a_point += s <= p and fold is not None
    assert public_with_a_point


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_per_slot_addition_uses_no_scratch(tmp_path):
    """The compiler's own metadata, read as tests/test_ptau_cpu.py reads it: group_add_each_kernel exists for G1 and for G2 and
    neither instance -- nor any other kernel of the translation unit -- keeps a stack frame."""
    out = tmp_path / "zkr_eval_tables.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "zkr_eval_tables.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    rows = {}
    for mt in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        rows[mt.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", mt.group(2)).group(1))
    inst = [k for k in rows if "group_add_each_kernel" in k]
    assert len(inst) == 2 and any("G1C" in k for k in inst) and any("G2C" in k for k in inst), inst
    assert any("group_inf_wire_kernel" in k for k in rows) and any("group_bitrev_kernel" in k for k in rows)
    assert {k: v for k, v in rows.items() if v} == {}
