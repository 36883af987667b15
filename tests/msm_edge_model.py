"""Integer model of the MSM's digit recoding and bucket geometry (csrc/kernels_msm.hpp, csrc/msm_plan.hpp), for the edge tests.

tests/test_gpu_msm_edges.py builds witnesses and scalar vectors that are meant to reach particular paths of the MSM: buckets
over `big_thresh`, more of them than BIG_CAP lists, more than BIG_SLOTS of them, buckets in the top size class, the
top-window spreading at every t.  Whether a vector really reaches a path depends on the plan, so the tests count it here
first, with the same rules the library uses; tests/test_msm_edge_model.py checks this model on the integers.
"""
import collections

import numpy as np

from bn254 import R

BIG_CAP = 1024            # kernels_msm.hpp: oversized buckets listed per MSM (the rest stay with msm_accum_kernel)
BIG_SLOTS = 64            # kernels_msm.hpp: oversized buckets per round of msm_big_body
SIZE_BINS = 1024          # kernels_msm.hpp: buckets of >= SIZE_BINS - 1 entries share the top size class
MAX_RANGES = 256          # msm_plan.hpp
SORT_RANGE_DEFAULT = 2048  # msm_plan.hpp
SORT_CHUNK_RECORDS = 3328  # msm_plan.hpp
MAX_FUSE = 16             # proofs one submit fuses at most (zkr_key_fuse of a 2^16 key)


def windows(c):
    """K = ceil(255 / c) windows of c bits (msm_plan)."""
    return (255 + c - 1) // c


def spread_tmax(c, K):
    """digit_spread_tmax: the t count of the top-window spreading, 0 when the top window never overflows."""
    bits = c * K - 1
    if bits <= 254:
        return 0
    if bits - 254 >= 12:
        return 4096
    return int(1.3225 * float(1 << (bits - 254)))   # the same double product, truncated, as the C++


def big_threshold(n, K, nbw, nbat=1):
    """big_threshold (msm_plan.hpp): occupancy above which a bucket goes to msm_big_kernel."""
    mean = n * K // nbw + 1
    by_bulk = (n * K * max(nbat, 1)) >> 17
    thr = min(by_bulk, mean * 8)
    thr = max(thr, 2 * mean)
    return max(thr, 64)


def plan(n_points, c):
    """The parts of msm_plan that decide which paths run, for window bits c and a table of n_points points."""
    K, nbw = windows(c), 1 << (c - 1)
    range_max = SORT_RANGE_DEFAULT
    if nbw // range_max > MAX_RANGES:
        range_max = nbw // MAX_RANGES
    nbl = min(nbw, range_max)
    nR = nbw // nbl
    J = (n_points * K + nR * SORT_CHUNK_RECORDS - 1) // (nR * SORT_CHUNK_RECORDS)
    return dict(c=c, K=K, nbw=nbw, nbl=nbl, nR=nR, J=max(1, min(64, J)), tmax=spread_tmax(c, K),
                big_thresh=big_threshold(n_points, K, nbw))


def spread_t(s, index, c, K, tmax):
    """t of DigitIter::init: index mod tmax when any bit at or above c (K - 1) is set, else 0."""
    return index % tmax if tmax > 1 and (s >> (c * (K - 1))) else 0


def digits_of(v, c, K):
    """DigitIter::next K times on v (= s + t r): the signed digits and what is left of v and the carry afterwards (both must
    be zero, or the digits do not rebuild v)."""
    mask, half = (1 << c) - 1, 1 << (c - 1)
    out, carry = [], 0
    for _ in range(K):
        raw = (v & mask) + carry
        v >>= c
        if raw > half:
            out.append(raw - (1 << c))
            carry = 1
        else:
            out.append(raw)
            carry = 0
    return out, v, carry


def recode(s, index, c, K, tmax):
    """(digits, t) of scalar s (< r) at position `index` of the digit kernels' vector."""
    t = spread_t(s, index, c, K, tmax)
    d, rest, carry = digits_of(s + t * R, c, K)
    assert rest == 0 and carry == 0, (c, s, t)
    return d, t


def occupancy(scalars, c, K, tmax, present=None, base_index=0):
    """Entries per bucket (bucket |d| - 1 of every non-zero digit) of the scalars whose points are `present`.  base_index:
    position of scalars[0] in the digit kernels' vector (a fused batch numbers the scalars of all its proofs end to end)."""
    tally = collections.Counter()
    for i, s in enumerate(scalars):
        if s and (present is None or present[i]):
            tally[(s, spread_t(s, base_index + i, c, K, tmax))] += 1
    counts = np.zeros(1 << (c - 1), dtype=np.int64)
    for (s, t), mult in tally.items():
        d, rest, carry = digits_of(s + t * R, c, K)
        assert rest == 0 and carry == 0
        for x in d:
            if x:
                counts[abs(x) - 1] += mult
    return counts


def paths(counts, thresh):
    """What one bucket set of these occupancies reaches: buckets over the threshold, how many of them the cap leaves to the
    accumulation at least, rounds of msm_big_body, buckets in the top size class among those over the threshold."""
    over = counts > thresh
    n_over = int(over.sum())
    return dict(over=n_over, over_cap=max(0, n_over - BIG_CAP), rounds=(min(n_over, BIG_CAP) + BIG_SLOTS - 1) // BIG_SLOTS,
                top_class=int((over & (counts >= SIZE_BINS - 1)).sum()), max=int(counts.max()) if counts.size else 0)


def group_sizes(count, cap):
    """How zkr_prove_batch cuts `count` proofs into fused submits (zkr_prove.hip group_count / next_group)."""
    if cap <= 1 or count <= 1:
        return [1] * count
    ng = (count + cap - 1) // cap
    if ng == 1 and 2 * count > cap:
        ng = 2
    out, left = [], count
    while ng:
        k = (left + ng - 1) // ng
        out.append(k)
        left -= k
        ng -= 1
    return out


# ---------------------------------------------------------------- scalars at the recoding's edges
def threshold(c, K):
    """2^(c (K - 1)): the smallest scalar whose top window is in play (and which is spread)."""
    return 1 << (c * (K - 1))


def all_digits(c, K, raw):
    """Sum of raw * 2^(c k) over as many windows as stay below r."""
    v = 0
    for k in range(K):
        w = v + (raw << (c * k))
        if w >= R:
            break
        v = w
    return v


def repeated_digit(c, K, d):
    """d in every window but the top one: K - 1 entries in bucket d - 1 (d <= 2^(c-1))."""
    return d * sum(1 << (c * k) for k in range(K - 1))


def carry_chain(c, K):
    """Window 0 = 2^(c-1) + 1 (a negative digit and a carry), windows 1 .. K-2 all ones: the carry runs to the top window."""
    return ((1 << c) - 1) * sum(1 << (c * k) for k in range(1, K - 1)) + (1 << (c - 1)) + 1


def edge_values(c, K):
    """The distinct edge scalars (< r) of a window geometry."""
    T = threshold(c, K)
    vals = {T - 1, T, T + 1, R - 1, R - 2, all_digits(c, K, 1 << (c - 1)), all_digits(c, K, (1 << (c - 1)) + 1),
            all_digits(c, K, (1 << c) - 1), carry_chain(c, K), T + carry_chain(c, K), R - 1 - carry_chain(c, K),
            repeated_digit(c, K, 1 << (c - 1)), (1 << 254) - 1 if (1 << 254) - 1 < R else R - 3}
    return sorted(v for v in vals if 0 < v < R)


def edge_vector(c, K, n, rnd):
    """n scalars (< r) for one window geometry: r - 1 at indices with t = tmax - 1 (the largest s + t r there is), the other
    edge values in turn at every third index, zeros, and random scalars between them."""
    tmax = spread_tmax(c, K)
    period = max(tmax, 1)
    vals = edge_values(c, K)
    out = [rnd.randrange(R) for _ in range(n)]
    for i in range(n):
        q, t = divmod(i, period)
        if (t == period - 1 and q % 2 == 0) if period > 1 else i % 7 == 1:
            out[i] = R - 1
        elif i % 3 == 0:
            out[i] = vals[(q + t) % len(vals)]
        elif i % 17 == 5:
            out[i] = 0
    return out
