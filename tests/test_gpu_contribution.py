"""A second party's delta contribution on the MI355X (zkr_key_contribute, zkr_key_contribution_verify, zkr_vk_contribute).

The oracle is exact: contribute(setup(t, alfa, beta, gamma, delta), d) must be the key setup(t, alfa, beta, gamma, delta d mod r)
produces, byte for byte -- every stored point is a canonical affine point and the arena layout depends on the key's contents
only.  Nothing in that comparison comes from the code under test except the contributed key and the patched verifying key.

Safety: the tampered keys (made as tests/test_gpu_key_check.py makes damaged arenas: save, patch bytes of the file, load) keep
every index a kernel follows; the only kernels that ever run on them are the checks.  Each is one call, run once."""

import os

import pytest

import groth16 as g
from test_gpu_key_check import T_A, T_C, T_H, _header
from test_rollup import as_inputs, scenario

pytestmark = pytest.mark.gpu

R = g.R
D = 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE
KEYSEC_POINTS, KEYSEC_COEF = 6, 8
TOX = ("t", "alfa", "beta", "gamma", "delta")


def _small():
    """The seeded m = 2^7 R1CS of tests/test_gpu_stages.py (conftest small_case), as zkr_setup_r1cs takes it."""
    import zkr_hip
    circ = g.synth_circuit(128, 7, 0x5A4B0001)
    cdef = dict(nVars=circ["nVars"], nPubInputs=5, nOutputs=2, constraints=[[{str(s): str(cf) for s, cf in lc} for lc in row] for row in circ["rows"]])
    w = circ["witness"]
    return zkr_hip.binarify_r1cs(cdef), g.binarify_witness(w), w[1:8], g.toxic_from_seed(0x5A4B00FF)


def _tx():
    """The reference's tx circuit, BatchProcessTx(2, 6): domain 2^17."""
    from zkr_hip import rollup as n
    c = n.RollupCircuit(2, 6)
    txs, _, _ = scenario(2, 6, 41, n_accounts=5)
    wb = c.calculate_witness(as_inputs(txs))
    return c.r1cs(), wb, c.public_signals(wb), g.toxic_from_seed(0x5A4B00F3)


def _setup(r1cs, tox, delta=None):
    import zkr_hip
    t = [tox[k] for k in TOX]
    if delta is not None:
        t[4] = delta
    return zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=t)


def _file(key, path):
    key.save(str(path))
    return open(path, "rb").read()


def _case(name, make, tmp_path_factory):
    r1cs, wb, pub, tox = make()
    k1, vk1 = _setup(r1cs, tox)
    k2, rec = k1.contribute(D)
    return dict(name=name, r1cs=r1cs, wb=wb, pub=pub, tox=tox, k1=k1, vk1=vk1, k2=k2, rec=rec, tmp=tmp_path_factory.mktemp("contrib_" + name))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    c = _case("small", _small, tmp_path_factory)
    yield c
    c["k2"].close()
    c["k1"].close()


@pytest.fixture(scope="module")
def tx(tmp_path_factory):
    c = _case("tx", _tx, tmp_path_factory)
    yield c
    c["k2"].close()
    c["k1"].close()


@pytest.fixture(params=["small", "tx"])
def case(request):
    return request.getfixturevalue(request.param)


def test_contributed_key_is_the_key_of_a_setup_with_delta_times_d(case):
    import zkr_hip
    k3, vk3 = _setup(case["r1cs"], case["tox"], case["tox"]["delta"] * D % R)
    f2, f3 = _file(case["k2"], case["tmp"] / "k2.zkr"), _file(k3, case["tmp"] / "k3.zkr")
    assert len(f2) == len(f3)
    assert f2 == f3
    assert _file(case["k1"], case["tmp"] / "k1.zkr") != f2
    vk2 = zkr_hip.vk_contribute(case["vk1"], case["rec"])
    assert vk2 == vk3
    rng = g.SplitMix64(4711)
    r, s = rng.fr(), rng.fr()
    p2, p3 = case["k2"].prove(case["wb"], r, s), k3.prove(case["wb"], r, s)
    assert len(p2) == 256 and p2 == p3
    k3.close()


def test_proofs_verify_under_the_contributed_vk_only_and_the_key_lives_like_any_other(case):
    import zkr_hip
    k1, k2, wb, pub = case["k1"], case["k2"], case["wb"], case["pub"]
    vk1, vk2 = case["vk1"], zkr_hip.vk_contribute(case["vk1"], case["rec"])
    rng = g.SplitMix64(31337)
    r, s = rng.fr(), rng.fr()
    p2, p1 = k2.prove(wb, r, s), k1.prove(wb, r, s)
    assert zkr_hip.verify(vk2, p2, pub) is True
    assert zkr_hip.verify(vk1, p2, pub) is False
    assert zkr_hip.verify(vk2, p1, pub) is False
    assert zkr_hip.verify(vk1, p1, pub) is True       # the source key is untouched and usable
    assert k2.check(level=1)["bad"] == 0
    assert k2.info() == k1.info() and k2.windows() == k1.windows()
    path = case["tmp"] / "k2_life.zkr"
    k2.save(str(path))
    kl = zkr_hip.ProvingKey.load_file(str(path))
    assert kl.prove(wb, r, s) == p2
    kl.close()
    kr = k2.replicate(k2.device)
    assert kr.prove(wb, r, s) == p2
    kr.close()
    shards = [k2.shard(0, 2), k2.shard(1, 2)]
    assert zkr_hip.prove_sharded(shards, wb, r, s) == p2
    for sh in shards:
        sh.close()


def test_verification_accepts_the_honest_pair(case):
    import zkr_hip
    assert zkr_hip.contribution_check(case["rec"]) is True
    assert case["k1"].contribution_verify(case["k2"], case["rec"]) == (True, 0, 0)


def _differing_pair(buf, off, count, size):
    """Indices i != j of two stored entries of `size` bytes that differ and are not all-zero (infinity placeholders)."""
    zero = bytes(size)
    ent = lambda i: buf[off + size * i: off + size * (i + 1)]
    i = next(k for k in range(count // 2, count) if ent(k) != zero)
    j = next(k for k in range(count // 4, count) if ent(k) != zero and ent(k) != ent(i))
    return i, j


def _tampered(case, name, patch):
    """k2's file with `patch(buf, header) -> [(offset, bytes)]` applied, loaded (level 0 runs at load and passes: no index moves)."""
    import zkr_hip
    buf = bytearray(_file(case["k2"], case["tmp"] / "k2_src.zkr"))
    h = _header(buf)
    for off, new in patch(buf, h):
        assert bytes(buf[off:off + len(new)]) != bytes(new)
        buf[off:off + len(new)] = new
    path = case["tmp"] / (name + ".zkr")
    open(path, "wb").write(buf)
    return zkr_hip.ProvingKey.load_file(str(path))


def _levels(h, t):
    return (255 + h["win_c"][t] - 1) // h["win_c"][t]


def _patch_coef(buf, h):
    off = h["off_coef"][0] + 32 * (h["nnz"][0] // 2)
    old = int.from_bytes(buf[off:off + 32], "little")
    return [(off, ((old + 1) % R).to_bytes(32, "little"))]        # another canonical value


def _patch_a_point(buf, h):
    i, j = _differing_pair(buf, h["off_pts"][T_A], h["npts"][T_A], 64)
    return [(h["off_pts"][T_A] + 64 * i, bytes(buf[h["off_pts"][T_A] + 64 * j: h["off_pts"][T_A] + 64 * (j + 1)]))]   # another point of the curve


def _patch_h_upper_level(buf, h):
    assert _levels(h, T_H) >= 2
    lvl = h["off_pts"][T_H] + 64 * h["npts"][T_H]                # level 1
    i, j = _differing_pair(buf, lvl, h["npts"][T_H], 64)
    return [(lvl + 64 * i, bytes(buf[lvl + 64 * j: lvl + 64 * (j + 1)]))]


def _patch_c_point_and_its_levels(buf, h):
    """C[i] <- C[j] at EVERY level: the levels stay the multiples of the base point, only the base point is wrong."""
    n = h["npts"][T_C]
    i, j = _differing_pair(buf, h["off_pts"][T_C], n, 64)
    out = []
    for k in range(_levels(h, T_C)):
        lvl = h["off_pts"][T_C] + 64 * n * k
        out.append((lvl + 64 * i, bytes(buf[lvl + 64 * j: lvl + 64 * (j + 1)])))
    return out


@pytest.mark.parametrize("name,patch,step,section", [
    ("qap_coefficient", _patch_coef, 3, KEYSEC_COEF),
    ("a_point", _patch_a_point, 3, KEYSEC_POINTS),
    ("h_upper_level", _patch_h_upper_level, 4, KEYSEC_POINTS),
    ("c_point_all_levels", _patch_c_point_and_its_levels, 5, 0),
])
def test_verification_refuses_a_tampered_key_and_names_the_step(small, name, patch, step, section):
    import zkr_hip
    case = small
    bad = _tampered(case, name, patch)
    try:
        if name == "h_upper_level":
            assert bad.check(level=1)["bad"] == 0     # zkr_key_check lets it through: the point IS on the curve
        assert case["k1"].contribution_verify(bad, case["rec"]) == (False, step, section)
        assert ("step %d" % step) in zkr_hip.lib().zkr_last_error().decode()
    finally:
        bad.close()


def test_verification_refuses_a_foreign_record_and_an_unmoved_key(case):
    k1, k2 = case["k1"], case["k2"]
    k2b, rec_b = k1.contribute(D + 2)
    ok, step, _ = k1.contribution_verify(k2, rec_b)              # a valid record, of another contribution
    assert (ok, step) == (False, 2)
    ok, step, _ = k1.contribution_verify(k1, case["rec"])        # delta did not move
    assert ok is False and step in (1, 2)
    assert k1.contribution_verify(k2b, rec_b) == (True, 0, 0)
    k2b.close()


def test_chained_contributions_with_drawn_secrets(case):
    import zkr_hip
    k2, rec = case["k2"], case["rec"]
    outs = [k2.contribute(None) for _ in range(2)]
    assert outs[0][1][64:128] != outs[1][1][64:128]              # two secrets, two delta1_after
    vk2 = zkr_hip.vk_contribute(case["vk1"], rec)
    for k3, rec3 in outs:
        assert rec3[:64] == rec[64:128]                          # chains on K2's delta1
        assert k2.contribution_verify(k3, rec3) == (True, 0, 0)
        vk3 = zkr_hip.vk_contribute(vk2, rec3)
        assert zkr_hip.verify(vk3, k3.prove(case["wb"]), case["pub"]) is True
        k3.close()


def test_refusals(case):
    import zkr_hip
    k1 = case["k1"]
    for d in (0, 1, R, R + 5, (1 << 256) - 1):
        with pytest.raises(zkr_hip.ZkrError) as e:
            k1.contribute(d)
        assert e.value.code == -5 and "1 < d < r" in str(e.value)
    sh = k1.shard(0, 2)
    with pytest.raises(zkr_hip.ZkrError) as e:
        sh.contribute(D)
    assert e.value.code == -5 and "shard" in str(e.value)
    with pytest.raises(zkr_hip.ZkrError) as e:
        k1.contribution_verify(sh, case["rec"])
    assert e.value.code == -5 and "shard" in str(e.value)
    sh.close()


def test_keys_on_different_devices_are_refused(case):
    import zkr_hip
    if zkr_hip.device_count() < 2:
        pytest.skip("needs two GPUs")
    other = case["k2"].replicate(1)
    with pytest.raises(zkr_hip.ZkrError) as e:
        case["k1"].contribution_verify(other, case["rec"])
    assert e.value.code == -5 and "devices" in str(e.value)
    other.close()


def test_contribution_at_2_20():
    """The memory plan where keys are 4.5 GB each: zkr_synth_key -> contribute -> contribution_verify -> a proof that verifies
    under zkr_synth_vk passed through zkr_vk_contribute."""
    import zkr_hip
    key, wb, aux = zkr_hip.ProvingKey.synth(20, 73, 0x5A4B0001, 0x5A4B00FF)
    vk = key.synth_vk(aux)
    pub = [int.from_bytes(wb[32 * i:32 * i + 32], "little") for i in range(1, 74)]
    k2, rec = key.contribute(None)
    assert key.contribution_verify(k2, rec) == (True, 0, 0)
    vk2 = zkr_hip.vk_contribute(vk, rec)
    proof = k2.prove(wb)
    assert zkr_hip.verify(vk2, proof, pub) is True and zkr_hip.verify(vk, proof, pub) is False
    k2.close()
    key.close()


def test_node_host_contributes_and_regenerates_the_verifier(tmp_path):
    """index.js: setup -> contribute({d}) switches the object's key -> the proof verifies under vkContribute(vkBin, record) only, is the
    closed form's proof for delta d, and solidityVerifyingKeySource of the new vkBin carries the new delta."""
    import json
    import shutil
    import subprocess
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simple-zk-rollups_amd")
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(pkg, "napi", "zkr_napi.node")):
        pytest.skip("node or the N-API addon is not available")
    circ = g.synth_circuit(128, 7, 0x5A4B0001)
    tox = g.toxic_from_seed(0x5A4B00FF)
    cdef = dict(nVars=circ["nVars"], nPubInputs=5, nOutputs=2, constraints=[[{str(s): str(cf) for s, cf in lc} for lc in row] for row in circ["rows"]])
    rng = g.SplitMix64(808)
    r, s = rng.fr(), rng.fr()
    path = tmp_path / "circ.json"
    path.write_text(json.dumps(dict(cdef=cdef, tox=[str(tox[k]) for k in TOX], witness=[str(x) for x in circ["witness"]], r=str(r), s=str(s), d=str(D))))
    script = """
      const z = require('./index.js'); const fs = require('fs');
      const d = JSON.parse(fs.readFileSync(process.argv[1]));
      (async () => {
        const bn = await z.buildBn128();
        const vk1 = bn.setup(d.cdef, {toxic: d.tox});
        const wb = z.binarifyWitness(d.witness), pub = d.witness.slice(1, 8);
        const {record} = bn.contribute({d: d.d});
        const vkBin2 = z.vkContribute(z.binarifyVerifyingKey(vk1), record);
        const vk2 = z.verifyingKeyFromBytes(vkBin2);
        const p2 = await bn.prove(wb, {r: d.r, s: d.s});
        const src1 = z.solidityVerifyingKeySource(z.binarifyVerifyingKey(vk1)), src2 = z.solidityVerifyingKeySource(vkBin2);
        console.log(JSON.stringify({p2, check: z.contributionCheck(record), ok2: z.isValid(vk2, p2, pub), ok1: z.isValid(vk1, p2, pub), len: record.length, srcMoved: src1 !== src2}));
      })().catch(e => { console.error(e); process.exit(1); });
    """
    run = subprocess.run([node, "-e", script, str(path)], cwd=pkg, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    res = json.loads(run.stdout)
    assert res["len"] == 352 and res["check"] is True and res["ok2"] is True and res["ok1"] is False and res["srcMoved"] is True
    tox2 = dict(tox, delta=tox["delta"] * D % R)
    assert res["p2"] == g.proof_to_json(g.proof_from_toxic(circ, tox2, circ["witness"], r, s))
