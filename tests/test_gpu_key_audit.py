"""zkr_key_audit on the MI355X: somebody who holds only the public artefacts -- circuit, transcript with its records, delta records,
proving key, verifying key -- decides whether the two keys are the ones the circuit and the transcript give, with delta moved only
by the recorded contributors.

Accepted: keys made by the library's own flow (zkr_setup_r1cs_ptau, then 0, 1 or 3 zkr_key_contribute calls), the same key
through a file and through its own websnark bytes, the smallest circuit, the reference's tx circuit.  Refused, each with its
step: the table that shows the equations bind -- a wrong tau, alfa or delta, broken record chains, one point of each table moved,
one window level, the verifying key's IC and delta, one coefficient of each side of the circuit, a damaged or a foreign
transcript.  Wherever the existing route (zkr_setup_r1cs_ptau + zkr_key_contribution_verify with every intermediate key, or a byte
comparison at zero contributions) can judge a refused key, it refuses it too.

Safety: the tampered keys are made as tests/test_gpu_contribution.py makes them (save, patch bytes of the file, load): every
index a kernel follows is kept, level 0 of zkr_key_check runs at load, only checks ever run on them, and each is audited once."""
import pytest

import groth16 as g
from test_gpu_contribution import _differing_pair, _file, _levels, _tampered
from test_gpu_key_check import T_A, T_B1, T_B2, T_C, T_H
from test_gpu_ptau import ALFA, ALFA1, ALFA2, BETA, BETA1, BETA2, TAU, TAU1, TAU2, _put

pytestmark = pytest.mark.gpu

R = g.R
D = 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE
SIZE = {T_A: 64, T_B1: 64, T_B2: 128, T_C: 64, T_H: 64}


def _r1cs(n_vars, n_pub_inputs, n_outputs, rows):
    import zkr_hip
    return zkr_hip.binarify_r1cs(dict(nVars=n_vars, nPubInputs=n_pub_inputs, nOutputs=n_outputs, constraints=[[{str(s): str(cf) for s, cf in lc} for lc in row] for row in rows]))


def _small_rows():
    """The rows of tests/test_gpu_contribution.py::_small, so that single coefficients can be changed."""
    return g.synth_circuit(128, 7, 0x5A4B0001)


def _transcript(K, secrets=((TAU1, ALFA1, BETA1), (TAU2, ALFA2, BETA2))):
    import zkr_hip
    t, recs = zkr_hip.ptau_new(K), []
    for s in secrets:
        t, r = zkr_hip.ptau_contribute(t, s)
        recs.append(r)
    return t, recs


def _last_error():
    import zkr_hip
    return zkr_hip.lib().zkr_last_error().decode()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Per transcript power: the transcript and its records, the key of the setup and the chain of three contributions after it
    (keys, records, verifying keys).  Power 7 with fixed d, power 9 with d drawn inside the library."""
    import zkr_hip
    circ = _small_rows()
    r1cs = _r1cs(circ["nVars"], 5, 2, circ["rows"])
    system = zkr_hip.ConstraintSystem.load(r1cs)
    w = dict(circ=circ, r1cs=r1cs, system=system, tmp=tmp_path_factory.mktemp("key_audit"))
    for K, ds in ((7, (D, D + 2, D + 4)), (9, (None, None, None))):
        ptau, precs = _transcript(K)
        k0, vk0 = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, ptau)
        keys, vks, recs = [k0], [vk0], []
        for d in ds:
            k, rec = keys[-1].contribute(d)
            keys.append(k)
            recs.append(rec)
            vks.append(zkr_hip.vk_contribute(vks[-1], rec))
        w[K] = dict(ptau=ptau, precs=precs, keys=keys, vks=vks, recs=recs)
    yield w
    for K in (7, 9):
        for k in w[K]["keys"]:
            k.close()
    system.close()


def _audit(w, K, key, n, **over):
    c = w[K]
    a = dict(system=w["system"], ptau=c["ptau"], ptau_records=c["precs"], delta_records=c["recs"][:n], vk_bin=c["vks"][n])
    a.update(over)
    return key.audit(a["system"], a["ptau"], a["ptau_records"], a["delta_records"], a["vk_bin"])


# ---------------------------------------------------------------- accepted
@pytest.mark.parametrize("n", [0, 1, 3])
@pytest.mark.parametrize("K", [7, 9], ids=["exact_power", "prefix_of_a_larger_transcript"])
def test_audit_accepts_the_keys_of_the_flow(world, K, n):
    res = _audit(world, K, world[K]["keys"][n], n)
    assert res == (True, 0, 0, 2, n), _last_error()
    assert res.valid is True and res.phase1_contributions == 2 and res.delta_contributions == n


def test_the_existing_route_accepts_the_honest_keys_too(world, tmp_path):
    """setup_r1cs_ptau again + a byte comparison for the key of the setup, contribution_verify with every intermediate key after it."""
    import zkr_hip
    c = world[7]
    again, vk = zkr_hip.ProvingKey.setup_r1cs_ptau(world["r1cs"], c["ptau"])
    try:
        assert _file(again, tmp_path / "again.zkr") == _file(c["keys"][0], tmp_path / "k0.zkr") and vk == c["vks"][0]
    finally:
        again.close()
    for j in range(3):
        assert c["keys"][j].contribution_verify(c["keys"][j + 1], c["recs"][j]) == (True, 0, 0)


def test_audit_accepts_the_final_key_through_a_file_and_through_its_websnark_bytes(world, tmp_path):
    """The websnark bytes make another arena from the same points: the audit reads points, not bytes."""
    import zkr_hip
    final = world[7]["keys"][3]
    path = tmp_path / "final.zkr"
    final.save(str(path))
    for other in (zkr_hip.ProvingKey.load_file(str(path)), zkr_hip.ProvingKey.load_websnark(final.to_websnark())):
        try:
            assert _audit(world, 7, other, 3) == (True, 0, 0, 2, 3), _last_error()
        finally:
            other.close()


def test_audit_accepts_the_smallest_circuit():
    """Two constraints, one public signal, written by hand: 2 + (1 + 1) appended rows = 4 rows, the domain 2^2 -- one butterfly
    level above the smallest transform, sums of four points, a B query with points at infinity.  The transcript has power 7."""
    import zkr_hip
    rows = [([(1, 1)], [(1, 1)], [(2, 1)]), ([(0, 3), (2, 1)], [(0, 1)], [(1, 1), (2, 1)])]
    r1cs = _r1cs(3, 0, 1, rows)
    ptau, precs = _transcript(7)
    system = zkr_hip.ConstraintSystem.load(r1cs)
    k0, vk0 = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, ptau)
    k1, rec = k0.contribute(D)
    try:
        info = k0.info()
        assert (info["nVars"], info["nPublic"], info["domainSize"]) == (3, 1, 4) and info["ptsB2"] < 3
        assert k0.audit(system, ptau, precs, [], vk0) == (True, 0, 0, 2, 0), _last_error()
        assert k1.audit(system, ptau, precs, [rec], zkr_hip.vk_contribute(vk0, rec)) == (True, 0, 0, 2, 1), _last_error()
    finally:
        k1.close()
        k0.close()
        system.close()


def test_audit_reads_wide_c_rows_through_the_wide_list():
    """A hand-written circuit whose second constraint has 70 terms on its C side (one wavefront, the stride loop taken twice by the
    first lanes) and 9 on the first (wide by one): accepted, and refused at step 8 when one coefficient in the tail of the long
    row changes -- the system's A and B sides still match the key's."""
    import zkr_hip
    n = 80
    rows = [([(1, 1)], [(2, 1)], [(s, s + 1) for s in range(3, 12)]),
            ([(2, 7), (0, 1)], [(1, 1)], [(s, 3 * s + 1) for s in range(5, 75)]),
            ([(3, 1)], [(4, 1)], [(5, 1)])]
    other = [rows[0], (rows[1][0], rows[1][1], rows[1][2][:68] + [(73, 5)] + rows[1][2][69:]), rows[2]]
    assert len(rows[1][2]) == 70 and other[1][2][68] != rows[1][2][68]
    r1cs = _r1cs(n, 0, 1, rows)
    ptau, precs = _transcript(7)
    system, changed = zkr_hip.ConstraintSystem.load(r1cs), zkr_hip.ConstraintSystem.load(_r1cs(n, 0, 1, other))
    k0, vk0 = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, ptau)
    try:
        assert k0.audit(system, ptau, precs, [], vk0) == (True, 0, 0, 2, 0), _last_error()
        assert changed.matches_key(k0) is True
        _refused(k0.audit(changed, ptau, precs, [], vk0), 8)
    finally:
        k0.close()
        changed.close()
        system.close()


def test_audit_accepts_the_tx_circuit_once():
    """BatchProcessTx(2, 6), domain 2^17, a power-17 transcript, one delta contribution."""
    import zkr_hip
    from zkr_hip import rollup as n
    r1cs = n.RollupCircuit(2, 6).r1cs()
    ptau, precs = _transcript(17, secrets=((TAU1, ALFA1, BETA1),))
    system = zkr_hip.ConstraintSystem.load(r1cs)
    k0, vk0 = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, ptau)
    k1, rec = k0.contribute(None)
    try:
        assert k1.audit(system, ptau, precs, [rec], zkr_hip.vk_contribute(vk0, rec)) == (True, 0, 0, 1, 1), _last_error()
    finally:
        k1.close()
        k0.close()
        system.close()


# ---------------------------------------------------------------- refused: keys that are not the transcript's
def _refused(res, step, detail=None):
    assert (res.valid, res.step) == (False, step), _last_error()
    if detail is not None:
        assert res.detail == detail, _last_error()
    assert ("step %d" % step) in _last_error()


@pytest.mark.parametrize("name,toxic,step,detail", [
    ("another_tau", [TAU + 1, ALFA, BETA, 1, 1], 6, T_A),
    ("only_alfa_differs", [TAU, ALFA + 1, BETA, 1, 1], 4, None),
    ("one_party_delta_and_no_records", [TAU, ALFA, BETA, 1, D], 3, None),
])
def test_audit_refuses_a_one_party_key_that_is_not_the_transcripts(world, tmp_path, name, toxic, step, detail):
    import zkr_hip
    key, vk = zkr_hip.ProvingKey.setup_r1cs(world["r1cs"], toxic=toxic)
    try:
        _refused(_audit(world, 7, key, 0, vk_bin=vk), step, detail)
        assert _file(key, tmp_path / "one_party.zkr") != _file(world[7]["keys"][0], tmp_path / "k0.zkr")      # the existing route: a byte comparison
    finally:
        key.close()


def test_audit_refuses_broken_delta_chains(world):
    c = world[7]
    k2, k3, recs = c["keys"][2], c["keys"][3], c["recs"]
    _refused(_audit(world, 7, k3, 3, delta_records=[recs[0], recs[2]]), 3, 1)          # the middle record removed: detail = its index
    k3b, rec3b = k2.contribute(D + 6)                                                  # another contribution of the same key
    try:
        assert rec3b[:64] == recs[1][64:128]
        _refused(_audit(world, 7, k3, 3, delta_records=[recs[0], recs[1], rec3b]), 3, 2)
        ok, step, _ = k2.contribution_verify(k3, rec3b)                                # the existing route
        assert (ok, step) == (False, 2)
    finally:
        k3b.close()


# ---------------------------------------------------------------- refused: tampered points
def _all_levels(t):
    def f(buf, h):
        n, size = h["npts"][t], SIZE[t]
        i, j = _differing_pair(buf, h["off_pts"][t], n, size)
        out = []
        for k in range(_levels(h, t)):
            lvl = h["off_pts"][t] + size * n * k
            out.append((lvl + size * i, bytes(buf[lvl + size * j: lvl + size * (j + 1)])))
        return out
    return f


def _upper_level_of_a(buf, h):
    assert _levels(h, T_A) >= 2
    lvl = h["off_pts"][T_A] + 64 * h["npts"][T_A]                # level 1
    i, j = _differing_pair(buf, lvl, h["npts"][T_A], 64)
    return [(lvl + 64 * i, bytes(buf[lvl + 64 * j: lvl + 64 * (j + 1)]))]


def _twiddle_entry(buf, h):
    """One entry of the key's twiddle table replaced by its neighbour: a canonical field element, so nothing a load checks."""
    off = h["off_tw"] + 32 * (h["m"] // 2)
    return [(off, bytes(buf[off + 32:off + 64]))]


TWIDDLES = 5      # report[1] at step 5 when the twiddle sections differ


@pytest.mark.parametrize("name,patch,step,detail", [
    ("twiddle_entry", _twiddle_entry, 5, TWIDDLES),
    ("a_point_all_levels", _all_levels(T_A), 6, T_A),
    ("b2_point_all_levels", _all_levels(T_B2), 6, T_B2),
    ("c_point_all_levels", _all_levels(T_C), 8, None),
    ("h_point_all_levels", _all_levels(T_H), 8, None),
    ("a_upper_level_only", _upper_level_of_a, 5, T_A),
])
def test_audit_refuses_a_tampered_key_and_names_the_step(world, name, patch, step, detail):
    c = world[7]
    bad = _tampered(dict(k2=c["keys"][3], tmp=world["tmp"]), name, patch)
    try:
        if name == "a_upper_level_only":
            assert bad.check(level=1)["bad"] == 0      # zkr_key_check lets it through: the point IS on the curve
        _refused(_audit(world, 7, bad, 3), step, detail)           # one audit, run once
        ok, _, _ = c["keys"][2].contribution_verify(bad, c["recs"][2])   # the existing route refuses it too
        assert ok is False
    finally:
        bad.close()


# ---------------------------------------------------------------- refused: the verifying key
def test_audit_refuses_a_verifying_key_with_two_ic_points_exchanged(world):
    vk = world[7]["vks"][3]
    ic1, ic2 = vk[452 + 64:452 + 128], vk[452 + 128:452 + 192]
    assert ic1 != ic2
    _refused(_audit(world, 7, world[7]["keys"][3], 3, vk_bin=_put(_put(vk, 452 + 64, ic2), 452 + 128, ic1)), 7)


def test_audit_refuses_a_verifying_key_with_the_delta_from_before_the_contributions(world):
    vk, vk0 = world[7]["vks"][3], world[7]["vks"][0]
    assert vk[320:448] != vk0[320:448]
    _refused(_audit(world, 7, world[7]["keys"][3], 3, vk_bin=_put(vk, 320, vk0[320:448])), 4)


# ---------------------------------------------------------------- refused: another circuit
def _changed(circ, side, public):
    """The circuit with ONE coefficient of `side` changed, on a public (s <= nPublic) or a private signal."""
    rows = [list(r) for r in circ["rows"]]
    for c, row in enumerate(rows):
        for k, (s, cf) in enumerate(row[side]):
            if (s <= circ["nPublic"]) == public:
                row[side] = row[side][:k] + [(s, (cf + 1) % R)] + row[side][k + 1:]
                return _r1cs(circ["nVars"], 5, 2, rows)
    raise AssertionError("no such term")


@pytest.mark.parametrize("name,side,public,step,same", [
    ("an_a_coefficient", 0, False, 2, False),
    ("a_c_coefficient_of_a_private_signal", 2, False, 8, True),      # the case zkr_r1cs_matches_key documents it cannot see
    ("a_c_coefficient_of_a_public_signal", 2, True, 7, True),
])
def test_audit_refuses_a_system_with_one_coefficient_changed(world, name, side, public, step, same):
    import zkr_hip
    system = zkr_hip.ConstraintSystem.load(_changed(world["circ"], side, public))
    try:
        assert system.matches_key(world[7]["keys"][3]) is same     # the hole ...
        _refused(_audit(world, 7, world[7]["keys"][3], 3, system=system), step)      # ... and its closing
    finally:
        system.close()


# ---------------------------------------------------------------- refused: another transcript
def test_audit_refuses_a_transcript_with_two_entries_of_alfa_tau_exchanged(world):
    ptau = world[7]["ptau"]
    o = 32 + 256 * 128                                             # alfaTauG1 of a power-7 transcript
    e3, e5 = ptau[o + 64 * 3:o + 64 * 4], ptau[o + 64 * 5:o + 64 * 6]
    _refused(_audit(world, 7, world[7]["keys"][3], 3, ptau=_put(_put(ptau, o + 64 * 3, e5), o + 64 * 5, e3)), 1)


def test_audit_refuses_a_valid_transcript_from_other_secrets(world):
    """Its own records verify (step 1) and the circuit is the key's (2), the delta chain is the key's (3): the constants come
    next, and alfa is not this transcript's -- step 4, before any sum is made (step 6 would say the same)."""
    ptau, precs = _transcript(7, secrets=((TAU1 + 1, ALFA1 + 1, BETA1 + 1), (TAU2, ALFA2, BETA2)))
    _refused(_audit(world, 7, world[7]["keys"][3], 3, ptau=ptau, ptau_records=precs), 4)


# ---------------------------------------------------------------- argument refusals
def test_audit_refuses_a_shard_and_a_wrong_ic_count(world):
    import zkr_hip
    sh = world[7]["keys"][3].shard(0, 2)
    try:
        with pytest.raises(zkr_hip.ZkrError) as e:
            _audit(world, 7, sh, 3)
        assert e.value.code == -5 and "shard" in str(e.value)
    finally:
        sh.close()
    vk = world[7]["vks"][3]
    short = vk[:448] + (7).to_bytes(4, "little") + vk[452:452 + 64 * 7]
    with pytest.raises(zkr_hip.ZkrError) as e:
        _audit(world, 7, world[7]["keys"][3], 3, vk_bin=short)
    assert e.value.code == -5 and "IC points" in str(e.value)


def test_audit_refuses_a_key_and_a_system_on_different_devices(world):
    import zkr_hip
    if zkr_hip.device_count() < 2:
        pytest.skip("needs two GPUs")
    other = world[7]["keys"][3].replicate(1)
    try:
        with pytest.raises(zkr_hip.ZkrError) as e:
            _audit(world, 7, other, 3)
        assert e.value.code == -5 and "device" in str(e.value)
    finally:
        other.close()
