"""zkr_key_export_websnark on the MI355X: a device key written back as the provingKeyBin of binarify.ts, for every way a whole key
comes to exist.

Everything is compared EXACTLY, as bytes.  The expected bytes never come from the export: they are the oracle's key
(groth16.setup + binarify_proving_key), the bytes zkr_setup_r1cs_websnark renders from the setup's own scalars (their pols sections, which
that writer and the export lay out with the same code, rebuilt here from the r1cs_bin), a patched copy of the oracle's key, or -- for the key of a ceremony, which no scalar-knowing writer can produce -- the proofs of the C oracle over
the exported bytes against the proofs of the key on the GPU.

Sizes: the export has ONE code path per group (a kernel thread per output point, in pieces of piece_points), so the cases are
the smallest that cross what can go wrong: a piece boundary inside a section and a ragged last piece (n = 128 with pieces of 1,
64, 100), more than one workgroup (2^10), identity and non-identity rank maps, the shared A / C layout and its placeholders, and
the rollup circuit for rows wider than the prover's wide-row threshold and a list of thousands of terms for signal 0."""
import json
import struct

import pytest

import coracle
import groth16 as g
from test_gpu_contribution import _small
from test_gpu_key_check import SPMV_WIDE, _header

pytestmark = pytest.mark.gpu

Q, R = g.Q, g.R
MONT = 1 << 256
ONE_Q = (MONT % Q).to_bytes(32, "little")
TAU1, ALFA1, BETA1 = 0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F7081, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978, 0x123456789ABCDEF0FEDCBA9876543210123456789ABCDEF
D1, D2 = 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE, 0x0DDBA11C0FFEE5EED0123456789ABCDEF0FEDCBA987654321


def _sections(pkb):
    n, p, m = struct.unpack_from("<3I", pkb, 0)
    ptr = list(struct.unpack_from("<7I", pkb, 12)) + [len(pkb)]
    return n, p, m, ptr


def _first_difference(a, b):
    if len(a) != len(b):
        return "lengths %d / %d" % (len(a), len(b))
    n, p, m, ptr = _sections(b)
    i = next(i for i in range(len(a)) if a[i] != b[i])
    names = ("polsA", "polsB", "A", "B1", "B2", "C", "hExps")
    sec = max((s for s in range(7) if ptr[s] <= i), default=None)
    return "byte %d (%s + %d)" % (i, "header" if sec is None else names[sec], i - (0 if sec is None else ptr[sec]))


def _same(got, want):
    assert got == want, _first_difference(got, want)


def _r1cs(circ, n_pub_inputs):
    import zkr_hip
    cdef = dict(nVars=circ["nVars"], nPubInputs=n_pub_inputs, nOutputs=circ["nPublic"] - n_pub_inputs,
                constraints=[[{str(s): str(cf) for s, cf in lc} for lc in row] for row in circ["rows"]])
    return zkr_hip.binarify_r1cs(cdef)


def _oracle_key(m, p, seed):
    circ = g.synth_circuit(m, p, seed)
    pk, _ = g.setup(circ, g.toxic_from_seed(seed ^ 0xFF))
    return g.binarify_proving_key(g.to_json_key(pk))


# ---------------------------------------------------------------- 1. bytes in, bytes out
def test_a_loaded_oracle_key_exports_its_own_bytes_m32():
    import zkr_hip
    pkb = _oracle_key(32, 3, 0x5A4B0011)
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    try:
        _same(key.to_websnark(), pkb)
    finally:
        key.close()


def test_a_loaded_oracle_key_exports_its_own_bytes_m128(small_case):
    import zkr_hip
    key = zkr_hip.ProvingKey.load_websnark(small_case["pkb"])
    try:
        _same(key.to_websnark(), small_case["pkb"])
    finally:
        key.close()


# ---------------------------------------------------------------- 2. against the writer that knows the scalars
def _pols_shape(pkb, s):
    """(terms per signal, terms per row) of side s of websnark bytes"""
    n, p, m, ptr = _sections(pkb)
    per_sig, per_row, o = [], [0] * m, ptr[s]
    for _ in range(n):
        (k,) = struct.unpack_from("<I", pkb, o)
        per_sig.append(k)
        for e in range(k):
            per_row[struct.unpack_from("<I", pkb, o + 4 + 36 * e)[0]] += 1
        o += 4 + 36 * k
    assert o == ptr[s + 1]
    return per_sig, per_row


def _pols_from_r1cs(r1cs):
    """polsA | polsB of the key of this r1cs_bin, rebuilt here: per signal its terms by row ascending (a row's in stored order,
    nothing merged or dropped), coefficient x 2^256 mod r, and on A the rows nConstraints + i that tie public signal i to itself"""
    n, p, n_c = struct.unpack_from("<3I", r1cs, 0)
    cols = [[[] for _ in range(n)] for _ in range(2)]
    o = 12
    for row in range(n_c):
        for s in range(3):
            (k,) = struct.unpack_from("<I", r1cs, o)
            o += 4
            for _ in range(k):
                if s < 2:
                    (sig,) = struct.unpack_from("<I", r1cs, o)
                    coef = int.from_bytes(r1cs[o + 4:o + 36], "little") * MONT % R
                    cols[s][sig].append(struct.pack("<I", row) + coef.to_bytes(32, "little"))
                o += 36
    assert o == len(r1cs)
    for i in range(p + 1):
        cols[0][i].append(struct.pack("<I", n_c + i) + (MONT % R).to_bytes(32, "little"))
    return b"".join(struct.pack("<I", len(terms)) + b"".join(terms) for side in cols for terms in side)


def _against_the_scalar_knowing_writer(r1cs, toxic):
    import zkr_hip
    want = zkr_hip.setup_r1cs_websnark(r1cs, toxic)[0]
    ptr = _sections(want)[3]
    assert want[ptr[0]:ptr[2]] == _pols_from_r1cs(bytes(r1cs))  # the setup's writer shares its front with the export: the pols are pinned here
    for side_tables in (True, False):
        key, _ = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=toxic, side_tables=side_tables)
        try:
            assert side_tables or key.h_form()["form"] == "coefficients"
            _same(key.to_websnark(), want)
        finally:
            key.close()
    return want


TOXIC = [0x1D0C5EED0123456789ABCDEF02468ACE13579BDF, 0x2468ACE013579BDF02468ACE13579BDF, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0, 0x5EED5EED5EED, 0x0CAFEBABEDEADBEEF0123456789ABCDEF]


def test_setup_key_exports_what_the_setup_renders_synthetic_2_10():
    circ = g.synth_circuit(1024, 73, 0x5A4B0001)
    pkb = _against_the_scalar_knowing_writer(_r1cs(circ, 70), TOXIC)
    assert _sections(pkb)[:3] == (circ["nVars"], 73, 1024)


def test_setup_key_exports_what_the_setup_renders_withdraw_circuit():
    from zkr_hip import rollup
    _against_the_scalar_knowing_writer(rollup.WithdrawCircuit().r1cs(), TOXIC)


def test_setup_key_exports_what_the_setup_renders_smallest_rollup_geometry():
    """BatchProcessTx(1, 1), the smallest geometry zkr_rollup_info accepts: rows wider than SPMV_WIDE (the wide-row lists of the
    arena are not empty) and a list for signal 0 -- the constant one -- far longer than any other."""
    import zkr_hip
    from zkr_hip import rollup
    with pytest.raises(zkr_hip.ZkrError):
        rollup.RollupCircuit(0, 1)
    with pytest.raises(zkr_hip.ZkrError):
        rollup.RollupCircuit(1, 0)
    pkb = _against_the_scalar_knowing_writer(rollup.RollupCircuit(1, 1).r1cs(), TOXIC)
    shapes = [_pols_shape(pkb, s) for s in range(2)]
    assert max(max(rows) for _, rows in shapes) > SPMV_WIDE
    for sigs, _ in shapes:
        assert sigs[0] > 1024 and sigs[0] > 4 * max(sigs[1:])


# ---------------------------------------------------------------- 3. pieces
def test_piece_boundaries_and_a_ragged_last_piece_change_nothing(small_case):
    import zkr_hip
    key = zkr_hip.ProvingKey.load_websnark(small_case["pkb"])
    try:
        assert key.info()["nVars"] == 128
        whole = key.to_websnark()
        _same(whole, small_case["pkb"])
        for piece in (1, 64, 100):
            _same(key.to_websnark(piece_points=piece), whole)
            assert key.export_times()["device_bytes"] == piece * 128
    finally:
        key.close()


# ---------------------------------------------------------------- 4. infinity, both table layouts
def _patched(pkb, c_fifth, y):
    """x = 0 (and y as given) for the first, the last and two middle entries of every section -- the same signals in A and C
    where C has them, so the two supports stay close -- and, with c_fifth, for every fifth entry of C as well"""
    n, p, m, ptr = _sections(pkb)
    b = bytearray(pkb)
    inf1, inf2 = bytes(32) + y, bytes(64) + y + bytes(32)

    def zero(t, i):
        if t == 2:
            b[ptr[4] + 128 * i:ptr[4] + 128 * i + 128] = inf2 if y != bytes(32) else bytes(128)
        else:
            b[ptr[2 + t] + 64 * i:ptr[2 + t] + 64 * i + 64] = inf1
    sigs = (0, n // 2, n // 2 + 1, n - 1)
    for s in sigs:
        for t in (0, 1, 2):
            zero(t, s)
    for i in {0, n - p - 2} | {s - p - 1 for s in sigs if s > p}:
        zero(3, i)
    for i in (0, m // 2, m // 2 + 1, m - 1):
        zero(4, i)
    if c_fifth:
        for i in range(0, n - p - 1, 5):
            zero(3, i)
    return bytes(b)


@pytest.mark.parametrize("c_fifth", [False, True], ids=["shared_a_c_layout", "separate_a_c_layout"])
def test_infinity_comes_out_as_the_reference_writes_it(small_case, c_fifth, tmp_path):
    import zkr_hip
    canon = _patched(small_case["pkb"], c_fifth, ONE_Q)
    assert canon != small_case["pkb"]
    key = zkr_hip.ProvingKey.load_websnark(canon)
    try:
        key.save(str(tmp_path / "k.zkr"))
        h = _header(open(tmp_path / "k.zkr", "rb").read())
        assert h["share_ac"] == (0 if c_fifth else 1)
        assert h["rank_identity"][0] == 0 and h["npts"][0] < h["n"]
        if not c_fifth:
            assert h["npts"][0] == h["npts"][3] > h["n"] - h["p"] - 1 - 5     # laid out over the union: placeholders in both
        _same(key.to_websnark(), canon)
        _same(key.to_websnark(piece_points=7), canon)
    finally:
        key.close()
    # the loader takes x = 0 alone as infinity: an input that writes it with y = 0 comes out with y = one
    key = zkr_hip.ProvingKey.load_websnark(_patched(small_case["pkb"], c_fifth, bytes(32)))
    try:
        _same(key.to_websnark(), canon)
    finally:
        key.close()


# ---------------------------------------------------------------- 5. the ceremony's key
def test_the_key_of_a_ceremony_reaches_the_reference_prover():
    import zkr_hip
    r1cs, wb, pub, _ = _small()
    ptau, _ = zkr_hip.ptau_contribute(zkr_hip.ptau_new(7), (TAU1, ALFA1, BETA1))
    k0, vk0 = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, ptau)
    k1, rec1 = k0.contribute(D1)
    key, rec2 = k1.contribute(D2)
    back = None
    try:
        vk1 = zkr_hip.vk_contribute(vk0, rec1)
        vk2 = zkr_hip.vk_contribute(vk1, rec2)
        pkx = key.to_websnark()
        rng = g.SplitMix64(20261021)
        r, s = rng.fr(), rng.fr()
        proof = key.prove(wb, r, s)
        assert coracle.prove(pkx, wb, r, s) == proof
        assert zkr_hip.verify(vk2, proof, pub) is True
        assert zkr_hip.verify(vk1, proof, pub) is False
        assert pkx != k1.to_websnark()
        back = zkr_hip.ProvingKey.load_websnark(pkx)
        assert back.prove(wb, r, s) == proof
        _same(back.to_websnark(), pkx)
    finally:
        for k in (back, key, k1, k0):
            if k is not None:
                k.close()


# ---------------------------------------------------------------- 6. origins
def test_every_origin_of_a_key_exports_the_sources_bytes(small_case, tmp_path):
    import zkr_hip
    r1cs = _small()[0]
    pkb = small_case["pkb"]
    src = zkr_hip.ProvingKey.load_websnark(pkb)
    made = [src]
    try:
        src.save(str(tmp_path / "k.zkr"))
        made.append(zkr_hip.ProvingKey.load_file(str(tmp_path / "k.zkr")))
        _same(made[-1].to_websnark(), pkb)
        for mode in ("full", "base"):
            made.append(src.replicate(0, mode=mode))
            assert made[-1].replication()["mode"] == mode
            _same(made[-1].to_websnark(), pkb)
        assert src.h_form()["form"] == "coefficients"
        assert src.eval_tables(r1cs) is True and src.h_form()["form"] == "evaluation"
        _same(src.to_websnark(), pkb)
    finally:
        for k in made:
            k.close()


# ---------------------------------------------------------------- 7. standard form
def _ints(v):
    if isinstance(v, str):
        return int(v) if v.isdigit() else v
    if isinstance(v, list):
        return [_ints(x) for x in v]
    return v


def test_the_json_key_binarifies_to_the_websnark_bytes(small_case):
    import zkr_hip
    key = zkr_hip.ProvingKey.load_websnark(_patched(small_case["pkb"], False, ONE_Q))
    try:
        jk = key.to_json_key()
        text = json.dumps(jk)
        assert json.loads(text) == jk
        assert jk["protocol"] == "groth" and jk["domainSize"] == 1 << jk["domainBits"] == 128
        assert jk["C"][:jk["nPublic"] + 1] == [None] * (jk["nPublic"] + 1) and jk["A"][0] == ["0", "1", "0"] and jk["B2"][0] == [["0", "0"], ["1", "0"], ["0", "0"]]
        assert jk["A"][1][2] == "1" and jk["B2"][1][2] == ["1", "0"] and all(isinstance(x, str) for x in jk["hExps"][1])     # finite in the oracle's key
        ints = {f: _ints(v) for f, v in jk.items() if not f.startswith("pols")}
        for f in ("polsA", "polsB"):
            ints[f] = [{int(c): int(v) for c, v in d.items()} for d in jk[f]]
        _same(g.binarify_proving_key(ints), key.to_websnark())
    finally:
        key.close()


# ---------------------------------------------------------------- 8. refusals and lifetime
def test_a_shard_is_refused_with_the_message(small_case):
    import zkr_hip
    key = zkr_hip.ProvingKey.load_websnark(small_case["pkb"])
    shard = key.shard(1, 2)
    try:
        with pytest.raises(zkr_hip.ZkrError) as e:
            shard.to_websnark()
        assert e.value.code == -5 and "a shard holds a range of the tables" in str(e.value)
    finally:
        shard.close()
        key.close()


def test_an_export_between_submit_and_collect_leaves_both_results_right(small_case):
    import torch
    import zkr_hip
    c = small_case
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    try:
        d_w = torch.frombuffer(bytearray(c["wb"]), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        want = coracle.prove(c["pkb"], c["wb"], c["r"], c["s"])
        ticket = key.prove_submit(d_w.data_ptr(), c["r"], c["s"])
        pkx = key.to_websnark()
        proof = key.prove_collect(ticket)
        assert proof == want
        _same(pkx, c["pkb"])
    finally:
        key.close()


def test_exports_leave_no_device_memory_behind(small_case):
    import torch
    import zkr_hip
    key = zkr_hip.ProvingKey.load_websnark(small_case["pkb"])
    try:
        key.to_websnark()
        torch.cuda.synchronize()
        free_after_first = torch.cuda.mem_get_info(0)[0]
        for _ in range(2):
            key.to_websnark()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free_after_first
    finally:
        key.close()
