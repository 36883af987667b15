"""CPU: the record of a delta contribution (zkr_contribution_check, zkr_vk_contribute: host only) against records assembled
here from known secrets with the oracle's point arithmetic (oracle/bn254.py) and the library's host MiMC sponge (pinned to the
oracle's and the reference's values by tests/test_rollup.py); and the code object of csrc/zkr_contribute.hip: no scratch."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

X, D, K = 0x1D0C5EED0123456789ABCDEF02468ACE13579BDF, 0x7E57AB1ED0D0CAFE, 0x0BADC0FFEE0DDF00D5EED  # delta = X g, the contribution, the nonce


def le(v):
    return int(v).to_bytes(32, "little")


def g1b(P):
    return le(P[0]) + le(P[1])


def g2b(P):
    return le(P[0][0]) + le(P[0][1]) + le(P[1][0]) + le(P[1][1])


def make_record(x=X, d=D, k=K, d_for_g2=None):
    """delta1_before | delta1_after | delta2_after | R | z, with z = k + c d and c the sponge over the ten coordinates."""
    import bn254 as b
    from zkr_hip import rollup as n
    d1b = b.g1_mul(b.G1_GEN, x)
    d1a = b.g1_mul(d1b, d)
    d2a = b.g2_mul(b.G2_GEN, x * (d if d_for_g2 is None else d_for_g2) % b.R)
    rp = b.g1_mul(d1b, k)
    c = n.multi_hash([d1b[0], d1b[1], d1a[0], d1a[1], d2a[0][0], d2a[0][1], d2a[1][0], d2a[1][1], rp[0], rp[1]])
    z = (k + c * d) % b.R
    return g1b(d1b) + g1b(d1a) + g2b(d2a) + g1b(rp) + le(z)


def twist_point_outside_g2():
    """On y^2 = x^3 + 3/(9+u) but not of order r (square root in Fq2 by the norm method, q = 3 mod 4)."""
    import bn254 as b

    def sqrt_fq(a):
        s = pow(a, (b.Q + 1) // 4, b.Q)
        return s if s * s % b.Q == a % b.Q else None

    def sqrt_fq2(a):
        a0, a1 = a
        s = sqrt_fq((a0 * a0 + a1 * a1) % b.Q)
        if s is None:
            return None
        for sg in (s, -s):
            x0 = sqrt_fq((a0 + sg) * b.inv(2) % b.Q)
            if x0:
                x1 = a1 * b.inv(2 * x0) % b.Q
                if b.f2sqr((x0, x1)) == (a0 % b.Q, a1 % b.Q):
                    return (x0, x1)
        return None
    k = 1
    while True:
        x = (k, 1)
        y = sqrt_fq2(b.f2add(b.f2mul(b.f2sqr(x), x), b.B2))
        k += 1
        if y is not None and b.g2_mul((x, y), b.R, reduce=False) is not None:
            assert b.g2_is_on_curve((x, y))
            return (x, y)


def test_record_from_known_secrets_passes_and_each_single_change_fails():
    import bn254 as b
    import zkr_hip
    rec = make_record()
    assert len(rec) == zkr_hip.CONTRIBUTION_BYTES == 352
    assert zkr_hip.contribution_check(rec) is True
    assert zkr_hip.contribution_check(make_record(x=5, d=2, k=1)) is True
    z = int.from_bytes(rec[320:], "little")
    other = b.g1_mul(b.G1_GEN, 0xABCDEF)
    bad = {
        "one bit of z": rec[:320] + le(z ^ (1 << 77)),
        "R another curve point": rec[:256] + g1b(other) + rec[320:],
        "delta2_after for a different d": make_record(d_for_g2=D + 1),
        "delta1_after = delta1_before": rec[:64] + rec[:64] + rec[128:],
        "a point off its curve": rec[:64] + rec[64:96] + le((int.from_bytes(rec[96:128], "little") + 1) % b.Q) + rec[128:],
        "G2 point outside the subgroup": rec[:128] + g2b(twist_point_outside_g2()) + rec[256:],
        "z >= r": rec[:320] + le(z + b.R),
    }
    assert z + b.R < 1 << 256
    for what, r in bad.items():
        assert len(r) == 352, what
        assert zkr_hip.contribution_check(r) is False, what
        assert "contribution record" in zkr_hip.lib().zkr_last_error().decode(), what
    # a record made with d = 1 moves nothing; one whose delta1_before is the point at infinity has no base
    assert zkr_hip.contribution_check(make_record(d=1)) is False
    assert zkr_hip.contribution_check(bytes(64) + rec[64:]) is False


def _vk(x):
    import bn254 as b
    ics = [b.g1_mul(b.G1_GEN, 11), b.g1_mul(b.G1_GEN, 12), b.g1_mul(b.G1_GEN, 13)]
    return (g1b(b.g1_mul(b.G1_GEN, 3)) + g2b(b.g2_mul(b.G2_GEN, 5)) + g2b(b.g2_mul(b.G2_GEN, 7)) + g2b(b.g2_mul(b.G2_GEN, x)) +
            len(ics).to_bytes(4, "little") + b"".join(g1b(p) for p in ics))


def test_vk_contribute_replaces_vk_delta_2_only_and_refuses_a_foreign_record():
    import bn254 as b
    import zkr_hip
    vk, rec = _vk(X), make_record()
    out = zkr_hip.vk_contribute(vk, rec)
    assert len(out) == len(vk)
    assert [i for i in range(len(vk)) if vk[i] != out[i]] != [] and all(320 <= i < 448 for i in range(len(vk)) if vk[i] != out[i])
    assert out[320:448] == g2b(b.g2_mul(b.G2_GEN, X * D % b.R)) == _vk(X * D % b.R)[320:448]
    assert out == _vk(X * D % b.R)
    # chaining: the next record starts where this one ended
    rec2 = make_record(x=X * D % b.R, d=0x5EC0BD, k=K + 1)
    assert rec2[:64] == rec[64:128]
    assert zkr_hip.vk_contribute(out, rec2) == _vk(X * D * 0x5EC0BD % b.R)
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.vk_contribute(_vk(X + 1), rec)      # delta1_before is not this key's delta
    assert e.value.code == -5 and "does not continue" in str(e.value)
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.vk_contribute(vk, rec[:320] + le(1))  # a record that does not verify
    assert e.value.code == -5
    with pytest.raises(zkr_hip.ZkrError):
        zkr_hip.vk_contribute(vk[:-1], rec)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_contribution_kernels_use_no_scratch(tmp_path):
    """The compiler's own metadata, read as tests/test_kernel_resources.py reads it: no kernel of zkr_contribute.hip spills or keeps a
    stack frame, and the scaling kernel (group_scale_uniform_kernel of kernels_group.hpp, instantiated here for G1 alone) leaves
    room for three wavefronts per SIMD: 168 VGPRs is the last allocation of 512 that does."""
    out = tmp_path / "zkr_contribute.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
                           "--cuda-device-only", "-S", os.path.join(ROOT, "simple-zk-rollups_amd", "csrc", "zkr_contribute.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    rows = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        g = lambda key: int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", m.group(2)).group(1))
        rows[m.group(1)] = (g("private_segment_fixed_size"), g("next_free_vgpr"))
    scale = [v for k, v in rows.items() if "group_scale_uniform_kernel" in k and "G1C" in k]
    assert len([k for k in rows if "group_scale_uniform_kernel" in k]) == 1
    assert len(scale) == 1 and any("compare_ranges_kernel" in k for k in rows)
    assert {k: v for k, v in rows.items() if v[0]} == {}
    assert scale[0][1] <= 168


NODE = shutil.which("node")
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")


@pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(PKG, "napi", "zkr_napi.node")), reason="node or the N-API addon is not available")
def test_node_host_checks_a_record_and_patches_a_vk():
    import bn254 as b
    vk, rec = _vk(X), make_record()
    script = """
      const z = require('./index.js');
      const vk = Buffer.from(process.argv[1], 'hex'), rec = Buffer.from(process.argv[2], 'hex'), bad = Buffer.from(rec);
      bad[330] ^= 1;
      let refused = '';
      try { z.vkContribute(vk, bad); } catch (e) { refused = String(e.message); }
      console.log(JSON.stringify({ok: z.contributionCheck(rec), bad: z.contributionCheck(bad), vk: Buffer.from(z.vkContribute(vk, rec)).toString('hex'), refused}));
    """
    r = subprocess.run([NODE, "-e", script, vk.hex(), rec.hex()], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout)
    assert res["ok"] is True and res["bad"] is False and "contribution record" in res["refused"]
    assert bytes.fromhex(res["vk"]) == _vk(X * D % b.R)
