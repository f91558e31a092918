"""The host twin of the device loop's random stream (workloads.philox4x32_10, md_deviate_uniforms, md_deviate) against what
is published and what can be computed exactly — no GPU and no library: the three known-answer vectors of philox4x32_10
(Random123's kat_vectors; Salmon et al., SC'11), the packing of (seed, t, atom, comp) into counter and key and of the output
words into the two uniforms, the edges of the uniforms, the float64 Box-Muller against mpmath at 40 digits, the distribution
(Kolmogorov distance to the normal law) and the independence of neighbours along each axis of the counter and of the key.
tests/test_hip_deviates.py then holds sgpr_md_deviates to this twin.

Measured: the twin differs from the 40-digit value by at most 2.08 units of 2^-52 r, r = sqrt(-2 ln u1), over the sample of
test_float64_twin_against_mpmath (the bound asserted there, 6 units, is reasoned in its docstring)."""
import math

import numpy as np
import pytest

from autoforce_amd.workloads import box_muller, md_deviate, md_deviate_uniforms, philox4x32_10, uniforms_of_words

TWO_PI_LITERAL = 6.283185307179586   # the angle factor of md_deviate: this double, not 2 pi

KAT = [   # counter, key -> output (Random123 kat_vectors, philox4x32 10 rounds)
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _words(s):
    return [int(w, 16) for w in s.split()]


def _signed64(x):
    return x - (1 << 64) if x >= 1 << 63 else x


@pytest.mark.parametrize("counter,key,out", KAT, ids=["zeros", "ones", "pi"])
def test_published_known_answers(counter, key, out):
    got = philox4x32_10(_words(counter), _words(key))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(w) for w in got] == _words(out), [f"{int(w):08x}" for w in got]


def test_known_answers_vectorised():
    """The three vectors in one call, and one key broadcast over several counters."""
    got = philox4x32_10([_words(c) for c, _, _ in KAT], [_words(k) for _, k, _ in KAT])
    assert got.tolist() == [_words(o) for _, _, o in KAT]
    both = philox4x32_10([[0, 0, 0, 0], [1, 0, 0, 0]], [0, 0])
    assert both.shape == (2, 4) and both[0].tolist() == _words(KAT[0][2]) and both[1].tolist() != both[0].tolist()


@pytest.mark.parametrize("counter,key,out", KAT, ids=["zeros", "ones", "pi"])
def test_known_answers_through_the_packing(counter, key, out):
    """(seed, t, atom, comp) built from the published words — t = c1 2^32 + c0 as a signed 64-bit word, seed = k1 2^32 + k0,
    atom = c2, comp = c3 as signed 32-bit words — must give the uniforms of the published output: u1 from words 0, 1 and u2
    from words 2, 3, 53 leading bits each.  A dropped high word of t or seed, exchanged atom and comp, exchanged output
    words or a shift other than 11 all miss the `pi` vector."""
    c, k, o = _words(counter), _words(key), _words(out)
    t, seed = _signed64(c[1] << 32 | c[0]), k[1] << 32 | k[0]
    atom, comp = (x - (1 << 32) if x >= 1 << 31 else x for x in c[2:])
    u1, u2 = md_deviate_uniforms(seed, t, atom, comp)
    e1 = (((o[0] << 32 | o[1]) >> 11) + 1) / 2 ** 53   # (integers below 2^53 over a power of two: exact in Python)
    e2 = ((o[2] << 32 | o[3]) >> 11) / 2 ** 53
    assert (float(u1), float(u2)) == (e1, e2), (float(u1), e1, float(u2), e2)


def test_high_words_of_seed_and_counter_count():
    """Seeds and t on both sides of 2^32 (and t < 0): the twin against philox4x32_10 fed words taken apart with Python
    integers, and different from what the low words alone give."""
    cases = [(1 << 32, 0), ((1 << 32) + 1, 5), (1 << 63, 1), ((1 << 64) - 1, 2), (77, 1 << 32), (77, (1 << 40) + 5), (77, (1 << 63) - 1),
             (77, -1), (77, -(1 << 63)), ((1 << 64) - 1, (1 << 63) - 3)]
    for seed, t in cases:
        tw = t & ((1 << 64) - 1)
        words = philox4x32_10([tw & 0xFFFFFFFF, tw >> 32, 9, 2], [seed & 0xFFFFFFFF, seed >> 32])
        u = md_deviate_uniforms(seed, t, 9, 2)
        assert tuple(map(float, u)) == tuple(map(float, uniforms_of_words(words))), (seed, t)
        low = md_deviate_uniforms(seed & 0xFFFFFFFF, tw & 0xFFFFFFFF, 9, 2)
        assert float(low[0]) != float(u[0]) and float(low[1]) != float(u[1]), (seed, t)
    a, b = md_deviate_uniforms(77, 3, 1, 2), md_deviate_uniforms(77, 3, 2, 1)
    assert float(a[0]) != float(b[0]) and float(a[1]) != float(b[1])   # atom and comp are different words of the counter


def test_word_order_into_the_uniforms():
    """Seed 77, t = atom = comp = 0 (worked out by hand from the rounds of md_deviate): which words make u1, which u2."""
    u1, u2 = md_deviate_uniforms(77, 0, 0, 0)
    assert float(u1) == 0.2061637303049435 and float(u2) == 0.7929304441361965, (float(u1), float(u2))
    x, r = float(md_deviate(77, 0, 0, 0)), math.sqrt(-2.0 * math.log(0.2061637303049435))
    assert abs(x - 0.47356936370220226) <= 16 * 2.0 ** -52 * r, (x, r)   # (two host libms: the tolerance of device against twin)


def test_uniform_edges():
    """All-zero words: u1 = 2^-53 (the smallest: the deviate is finite, r = sqrt(106 ln 2)) and u2 = 0; all-one words: u1 = 1
    (the deviate is exactly 0) and u2 = 1 - 2^-53 < 1.  The eleven dropped bits do not matter."""
    u1, u2 = uniforms_of_words([0, 0, 0, 0])
    assert float(u1) == 2.0 ** -53 and float(u2) == 0.0
    x = float(box_muller(u1, u2))
    r = math.sqrt(106.0 * math.log(2.0))
    assert math.isfinite(x) and abs(x - r) <= 4 * 2.0 ** -52 * r and 8.5 < x < 8.6, x
    u1, u2 = uniforms_of_words([0xFFFFFFFF] * 4)
    assert float(u1) == 1.0 and float(u2) == 1.0 - 2.0 ** -53 and float(u2) < 1.0
    assert float(box_muller(u1, u2)) == 0.0
    assert tuple(map(float, uniforms_of_words([0, 0x7FF, 0, 0x7FF]))) == (2.0 ** -53, 0.0)
    assert tuple(map(float, uniforms_of_words([0, 0x800, 0, 0x800]))) == (2.0 ** -52, 2.0 ** -53)
    assert tuple(map(float, uniforms_of_words([0xFFFFFFFF, 0xFFFFF7FF, 1, 0]))) == (1.0 - 2.0 ** -53, 2.0 ** -32)
    u1, u2 = md_deviate_uniforms(np.arange(1, 5)[:, None], np.arange(1000)[None, :], 3, 1)
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0


def test_float64_twin_against_mpmath():
    """The float64 Box-Muller of the twin against mpmath at 40 digits, u1 and u2 taken as the exact doubles they are and the
    angle factor as the same double literal, in units of 2^-52 r with r = sqrt(-2 ln u1): 4096 deviates in stream order plus,
    from 2 10^5 more, the 64 with the largest r and the 64 each with |cos| nearest 0 and nearest 1, and the two edge values
    of u1.  Bound, with log and cos of the host good to 2 units in the last place (glibc states less than 1, numpy's vector
    loops a few) and sqrt and the products correctly rounded: the angle fl(tau u2) < 8 is off by at most 2^-51, which moves
    cos by at most 2 units; cos itself 2; log, halved by the square root, 1; the square root 1/2; the last product 1/2 — 6
    units.  (Nearest |cos| = 1 the first term vanishes, nearest 0 it is the whole error: r |sin| dtheta.)"""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    t, a, c = np.arange(1366)[:, None, None], np.arange(50)[None, :, None], np.arange(3)[None, None, :]
    u1, u2 = (u.ravel() for u in md_deviate_uniforms(77, t, a, c))
    cosv = np.abs(np.cos(TWO_PI_LITERAL * u2))
    pick = np.unique(np.concatenate([np.arange(4096), np.argsort(u1)[:64], np.argsort(cosv)[:64], np.argsort(cosv)[-64:]]))
    u1 = np.concatenate([u1[pick], [2.0 ** -53, 1.0, 2.0 ** -53, 1.0 - 2.0 ** -53]])
    u2 = np.concatenate([u2[pick], [0.0, 0.3, 1.0 - 2.0 ** -53, 0.25]])
    got = box_muller(u1, u2)
    tau = mpmath.mpf(TWO_PI_LITERAL)
    worst = (0.0, None)
    for x, p, q in zip(got.tolist(), u1.tolist(), u2.tolist()):
        r = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(p)))
        exact = r * mpmath.cos(tau * mpmath.mpf(q))
        if r == 0:
            assert x == 0.0
            continue
        units = float(abs(mpmath.mpf(x) - exact) / (r * mpmath.mpf(2) ** -52))
        if units > worst[0]:
            worst = (units, (p, q, x))
    print(f"twin against mpmath: {len(got)} deviates, largest error {worst[0]:.3f} units of 2^-52 r at (u1, u2, value) = {worst[1]}")
    assert worst[0] <= 6.0, worst


def _grid(seeds):
    """X[s, t, a, c] over 4 seeds x 25 configurations x 334 atoms x 3 components (100 200 deviates)."""
    s = np.array(seeds, dtype=np.uint64)[:, None, None, None]
    return md_deviate(s, np.arange(25)[None, :, None, None], np.arange(334)[None, None, :, None], np.arange(3)[None, None, None, :])


def test_distribution_is_standard_normal():
    """Kolmogorov distance to Phi of n = 10^5 deviates (the first 10^5 of 4 seeds x t x atom x comp in that order) under the
    Dvoretzky-Kiefer-Wolfowitz bound at alpha = 10^-6: sqrt(ln(2 / alpha) / (2 n)) = 0.0085.  Fixed inputs: it cannot flake."""
    n = 100_000
    x = np.sort(_grid([1, 77, (1 << 32) + 1, (1 << 64) - 1]).ravel()[:n])
    phi = 0.5 * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))
    k = np.arange(1, n + 1)
    dist = max(float(np.max(k / n - phi)), float(np.max(phi - (k - 1) / n)))
    bound = math.sqrt(math.log(2.0 / 1e-6) / (2.0 * n))
    print(f"Kolmogorov distance {dist:.5f}, bound {bound:.5f}; mean {x.mean():+.5f}, std {x.std():.5f}, largest |x| {np.abs(x).max():.3f}")
    assert 0.0084 < bound < 0.0086 and dist <= bound, (dist, bound)
    assert np.all(np.isfinite(x))


def test_neighbours_along_each_axis_are_uncorrelated():
    """Sample correlation of each deviate with its neighbour in t, in atom, in comp, and in the seed (s and s + 1), each
    axis by itself, under 5 / sqrt(number of pairs)."""
    X = _grid([77, 78, 79, 80])
    for axis, name in enumerate(("seed", "t", "atom", "comp")):
        lo, hi = [slice(None)] * 4, [slice(None)] * 4
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        a, b = X[tuple(lo)].ravel(), X[tuple(hi)].ravel()
        rho = float(np.corrcoef(a, b)[0, 1])
        print(f"neighbours in {name}: correlation {rho:+.5f} over {a.size} pairs, bound {5.0 / math.sqrt(a.size):.5f}")
        assert abs(rho) < 5.0 / math.sqrt(a.size), (name, rho)
