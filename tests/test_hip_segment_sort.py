"""The segment sort at the head of the row collapse on the GPU, through rpvg_hip_segment_sort_words: the device routines and
launches of the collapse (small kernel, chunk kernel, merge rounds, read-back of every segment from its own final buffer) on
words of the test's own, against numpy.sort per segment.

The entry writes the sorted words only: what the collapse derives from a word and its predecessor in the image ("equal to its
predecessor", the stretch starts, also across lane and wavefront boundaries) is not checked here but by tests/test_hip_collapse.py,
whose planted rows go through the one-wavefront, two-wavefront and chunked routes, and row by row by tests/test_hip_collapse_edges.py,
whose runs and stretches of bit-identical rows lie across the sorted positions 64, 512, 1 024 and 2 048."""
import numpy as np
import pytest

from rpvg_amd import hip

pytestmark = pytest.mark.gpu

CHUNK = 2048  # rpvg_sort::kChunkRows
SMALL = [0, 1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025]
CHUNKED = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 5 * CHUNK + 3, 9 * CHUNK - 7]
SIZES = SMALL + CHUNKED


def _words(rng, n, kind):
    """n distinct words below 2^64 - 1: random, or differing in their low / high halves only; 0xFF..FE among them."""
    part = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(2 ** 32))
    if kind == "low":
        w = np.uint64(0x0123456700000000) | part
    elif kind == "high":
        w = (part << np.uint64(32)) | np.uint64(0x89ABCDEF)
    else:
        w = (rng.integers(0, 2 ** 63, size=n, dtype=np.uint64) << np.uint64(1) & ~np.uint64(0xFFFFFF)) | rng.permutation(n).astype(np.uint64)
    if n >= 2:
        w[int(rng.integers(n))] = np.uint64(0xFFFFFFFFFFFFFFFE)
    assert len(np.unique(w)) == n and (n == 0 or int(w.max()) < 2 ** 64 - 1)
    return w


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def segments():
    rng = np.random.default_rng(20240611)
    kinds = ["random", "low", "high"]
    return [_words(rng, n, kinds[i % 3]) for i, n in enumerate(SIZES)]


def _sort(ctx, segs):
    off = np.zeros(len(segs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in segs])
    words = np.concatenate(segs) if segs else np.zeros(0, dtype=np.uint64)
    out = ctx.segment_sort_words(words, off)
    return out, [out[int(off[i]):int(off[i + 1])] for i in range(len(segs))]


def _check(segs, got):
    for s, g in zip(segs, got):
        assert np.array_equal(g, np.sort(s)), len(s)


def test_mixed_call_sorts_every_segment_and_repeats_its_bytes(ctx, segments):
    out, got = _sort(ctx, segments)
    _check(segments, got)
    again, _ = _sort(ctx, segments)
    assert out.tobytes() == again.tobytes()


def test_mixed_call_with_the_segments_in_reverse_order(ctx, segments):
    segs = segments[::-1]
    _check(segs, _sort(ctx, segs)[1])


@pytest.mark.parametrize("n", CHUNKED)
def test_a_chunked_segment_alone(ctx, segments, n):
    """alone, the rounds launched are the rounds this segment needs: the mixed call launches four whatever the segment"""
    segs = [segments[SIZES.index(n)]]
    _check(segs, _sort(ctx, segs)[1])


def test_low_and_high_halves_in_every_size_class(ctx):
    rng = np.random.default_rng(7)
    segs = [_words(rng, n, kind) for n in (64, 128, 256, 512, 1024, CHUNK, 3 * CHUNK + 5) for kind in ("low", "high")]
    _check(segs, _sort(ctx, segs)[1])
