"""CPU: the integer model of the MSM's digit recoding and bucket geometry (tests/msm_edge_model.py) that
tests/test_gpu_msm_edges.py relies on to know which paths its vectors reach."""
import random

import numpy as np
import pytest

import msm_edge_model as em
from bn254 import R

ALL_C = range(2, 23)   # every window size ZKR_MSM_C accepts


@pytest.mark.parametrize("c", ALL_C)
def test_spread_bound_holds_for_the_mirrored_tmax(c):
    """tmax r <= 2^(cK - 1): every s + t r with s < r and t < tmax keeps its top signed digit in range.  tmax is the largest such
    count below the 4096 cap, and the classes the issue names are the ones the plan gives."""
    K = em.windows(c)
    tmax = em.spread_tmax(c, K)
    if tmax:
        assert tmax * R <= 1 << (c * K - 1)
        if tmax < 4096:
            assert (tmax + 1) * R > 1 << (c * K - 1)      # the largest count, not merely a safe one
    else:
        assert c * K - 1 <= 254
    assert tmax == {3: 0, 5: 0, 15: 0, 17: 0, 2: 2, 4: 2, 8: 2, 16: 2, 18: 4096, 21: 4096}.get(c, tmax)


@pytest.mark.parametrize("c", ALL_C)
def test_signed_digits_rebuild_every_edge_scalar(c):
    """For every edge scalar at every t in 0 .. tmax - 1 (and random scalars): the modelled digits lie in
    (-2^(c-1), 2^(c-1)], nothing is left over after K windows, and sum d_k 2^(ck) = s + t r."""
    K = em.windows(c)
    tmax = em.spread_tmax(c, K)
    rnd = random.Random(c)
    half = 1 << (c - 1)
    vals = em.edge_values(c, K) + [rnd.randrange(R) for _ in range(20)] + [1, 2, half, half + 1]
    ts = sorted({0, 1, tmax // 2, tmax - 1} & set(range(max(tmax, 1)))) if tmax > 64 else range(max(tmax, 1))
    for s in vals:
        for t in ts:
            d, rest, carry = em.digits_of(s + t * R, c, K)
            assert rest == 0 and carry == 0, (s, t)
            assert all(-half < x <= half for x in d), (s, t)
            assert sum(x << (c * k) for k, x in enumerate(d)) == s + t * R
        # the recoding the kernels do at an index of class tmax - 1
        d, t = em.recode(s, max(tmax, 1) * 3 + max(tmax - 1, 0), c, K, tmax)
        assert t == (max(tmax - 1, 0) if tmax > 1 and s >= em.threshold(c, K) else 0)
        assert sum(x << (c * k) for k, x in enumerate(d)) == s + t * R


@pytest.mark.parametrize("c", ALL_C)
def test_edge_scalars_are_what_they_claim(c):
    K = em.windows(c)
    T, half = em.threshold(c, K), 1 << (c - 1)
    vals = em.edge_values(c, K)
    assert all(0 < v < R for v in vals)
    if T < R:
        assert T in vals and T - 1 in vals
    else:                                                                                 # c = 2: 2^254 > r, nothing is spread
        assert c == 2 and not any(em.spread_t(v, 1, c, K, 2) for v in vals)
    assert em.spread_t(T, 5, c, K, 7) == 5 % 7 and em.spread_t(T - 1, 5, c, K, 7) == 0      # where `hi` flips
    d, _, _ = em.digits_of(em.all_digits(c, K, half), c, K)
    assert d[0] == d[1] == half                                                           # bucket nbw - 1
    d, _, _ = em.digits_of(em.carry_chain(c, K), c, K)
    assert d[0] == -(half - 1) and all(x == 0 for x in d[1:K - 1]) and d[K - 1] == 1       # carry from window 0 to the top
    d, _, _ = em.digits_of(em.repeated_digit(c, K, min(3, half)), c, K)
    assert d == [min(3, half)] * (K - 1) + [0]                                            # K - 1 entries in one bucket
    tmax = em.spread_tmax(c, K)
    vec = em.edge_vector(c, K, max(600, tmax + 1), random.Random(c))
    if tmax > 1 and T < R:
        assert vec[tmax - 1] == R - 1 and em.spread_t(vec[tmax - 1], tmax - 1, c, K, tmax) == tmax - 1


def test_occupancy_and_thresholds_on_small_cases():
    """occupancy() against a plain digit count; big_threshold / plan / group_sizes against values worked out by hand from the
    C++ (msm_plan.hpp big_threshold and msm_plan, zkr_prove.hip group_count)."""
    rnd = random.Random(9)
    for c in (2, 3, 5, 9, 16):
        K = em.windows(c)
        tmax = em.spread_tmax(c, K)
        sc = em.edge_vector(c, K, 300, rnd)
        present = np.array([i % 5 != 2 for i in range(300)])
        want = np.zeros(1 << (c - 1), dtype=np.int64)
        for i, s in enumerate(sc):
            if present[i]:
                for x in em.recode(s, 1000 + i, c, K, tmax)[0]:
                    if x:
                        want[abs(x) - 1] += 1
        assert (em.occupancy(sc, c, K, tmax, present, base_index=1000) == want).all()
    # 2^20 rollup-shaped key (A table ~ 0.97 M points): c = 20, K = 13, 2^19 buckets
    assert em.big_threshold(1013000, 13, 1 << 19) == 100
    assert em.big_threshold(100, 85, 4) == 2 * (100 * 85 // 4 + 1)       # dense little bucket sets: twice the mean
    assert em.big_threshold(65000, 16, 1 << 15, 16) == (65000 * 16 * 16) >> 17
    p = em.plan(1 << 20, 20)
    assert (p["K"], p["nbw"], p["nR"], p["nbl"], p["tmax"]) == (13, 1 << 19, 256, 2048, 42)
    p = em.plan(80000, 22)
    assert (p["nR"], p["nbl"], p["J"]) == (256, 8192, 2)
    assert em.group_sizes(19, 16) == [10, 9] and em.group_sizes(16, 16) == [8, 8] and em.group_sizes(7, 16) == [7]
    assert em.group_sizes(50, 8) == [8, 7, 7, 7, 7, 7, 7] and em.group_sizes(3, 1) == [1, 1, 1]
    pth = em.paths(np.array([5000] * 1100 + [70] * 10 + [0] * 30), 64)
    assert pth == dict(over=1110, over_cap=86, rounds=16, top_class=1100, max=5000)
