"""CPU: the device-free half of the regrouped shadow-ray kernel (restir_amd/csrc/rs_shadow_regroup.h) through rs_debug_plan_shadow_regroup:
shadow_bin -- which of 64 length bins a segment lies in -- on hand rows and on its properties, and the slot plan of a block of 256 lanes
against a NumPy restatement.  A wrong bin or a wrong first slot changes no pixel by itself (any assignment of rays to lanes gives the same
occlusion), but slots that are no permutation would lose or repeat a ray, and a conversion of an unclamped length is undefined.
tools/models/shadow_regroup_plan.cpp runs the same cases under AddressSanitizer + UBSan."""
import numpy as np
import pytest

from restir_amd import capi

BINS = 64
INF, NAN = np.float32(np.inf), np.float32(np.nan)
ROOT = (np.array([-1.0, 0.0, 2.0], np.float32), np.array([2.0, 4.0, 14.0], np.float32))          # a diagonal of 13


def bins_of(lengths, k=None, root=None):
    return capi.plan_shadow_regroup(lengths, bins_over_extent=k, root=root)[0]


def test_the_scale_is_the_bins_over_the_root_diagonal():
    _, k = capi.plan_shadow_regroup([1.0], root=ROOT)
    assert np.float32(k) == np.float32(64.0) / np.float32(13.0)


def test_hand_rows():
    k = np.float32(64.0) / np.float32(13.0)
    tiny = np.float32(1e-45)            # the smallest subnormal
    assert tiny > 0 and tiny == np.nextafter(np.float32(0), np.float32(1))
    rows = [(0.0, 0), (-0.0, 0), (tiny, 0), (-1.0, 0), (-1e30, 0), (-INF, 0),
            (13.0, 63), (26.0, 63), (1e10, 63), (3.4e38, 63), (INF, 63), (NAN, 63)]
    got = bins_of([r[0] for r in rows], root=ROOT)
    assert got.tolist() == [r[1] for r in rows]
    assert bins_of([r[0] for r in rows], k=k).tolist() == got.tolist()


@pytest.mark.parametrize("edge", [1, 2, 7, 31, 62, 63])
def test_bin_edges(edge):
    """With 4 bins per unit of length the edges are exact floats: the edge opens its bin, the float below it closes the one before."""
    at = np.float32(edge * 0.25)
    below = np.nextafter(at, np.float32(0))
    assert bins_of([below, at], k=4.0).tolist() == [edge - 1, edge]


def test_the_top_bin_takes_everything_from_its_edge_on():
    assert bins_of([np.nextafter(np.float32(15.75), np.float32(0)), 15.75, 16.0, 32.0], k=4.0).tolist() == [62, 63, 63, 63]


def test_a_degenerate_root_box_has_defined_bins():
    p = np.ones(3, np.float32)
    b, k = capi.plan_shadow_regroup([0.0, 1.0, -1.0, 1e10], root=(p, p))
    assert np.isinf(k) and b.tolist() == [63, 63, 0, 63]            # 0 * inf is a NaN: the top bin


def test_monotone_and_in_range():
    rng = np.random.default_rng(5)
    lengths = np.concatenate([rng.uniform(-2, 20, 100_000 - 6), [0.0, 1e10, np.inf, -np.inf, 13.0, 12.999]]).astype(np.float32)
    lengths.sort()
    b = bins_of(lengths, root=ROOT)
    assert b.min() == 0 and b.max() == BINS - 1
    assert np.all(np.diff(b) >= 0)
    finite = np.isfinite(lengths) & (lengths >= 0) & (lengths < 12.7)
    k = np.float32(64.0) / np.float32(13.0)
    assert np.array_equal(b[finite], np.floor(lengths[finite] * k).astype(np.int32))
    assert np.all(bins_of(np.append(lengths, NAN), root=ROOT)[-1:] == BINS - 1)


# ---- the slot plan -------------------------------------------------------------------------------------------------------------------------
def numpy_plan(bins, active):
    """first[b] = the active rays in bins above b; count = the active rays."""
    hist = np.bincount(np.asarray(bins)[np.asarray(active, bool)], minlength=BINS)
    above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])
    return above.astype(np.int32), int(hist.sum())


def check_plan(bins, active):
    bins = np.asarray(bins, np.int32); active = np.asarray(active, bool)
    lengths = (bins.astype(np.float32) + np.float32(0.5)) * np.float32(0.25)           # bin b under 4 bins per unit
    got_bins, _, first, count = capi.plan_shadow_regroup(lengths, bins_over_extent=4.0, active=active, plan=True)
    assert np.array_equal(got_bins, bins)
    want_first, want_count = numpy_plan(bins, active)
    assert count == want_count and np.array_equal(first, want_first)
    # slots handed out first[bin]++ in any arrival order: a permutation of 0 .. count - 1, descending in bin
    nxt = first.copy(); slot_bin = np.full(count, -1)
    for i in np.random.default_rng(int(bins.sum()) + count).permutation(len(bins)):
        if active[i]:
            s = nxt[bins[i]]; nxt[bins[i]] += 1
            assert 0 <= s < count and slot_bin[s] < 0
            slot_bin[s] = bins[i]
    assert np.all(slot_bin >= 0) and np.all(np.diff(slot_bin) <= 0)


def test_plan_all_inactive():
    check_plan(np.arange(256) % BINS, np.zeros(256, bool))
    _, _, first, count = capi.plan_shadow_regroup(np.ones(256, np.float32), bins_over_extent=4.0, active=np.zeros(256), plan=True)
    assert count == 0 and not first.any()


def test_plan_one_active():
    active = np.zeros(256, bool); active[200] = True
    check_plan(np.full(256, 17), active)


@pytest.mark.parametrize("b", [0, 31, 63])
def test_plan_all_in_one_bin(b):
    check_plan(np.full(256, b), np.ones(256, bool))
    _, _, first, count = capi.plan_shadow_regroup(np.full(256, (b + 0.5) * 0.25, np.float32), bins_over_extent=4.0, plan=True)           # active=None: all
    assert count == 256 and first[b] == 0 and np.all(first[:b] == 256) and np.all(first[b + 1:] == 0)


def test_plan_256_distinct_lengths():
    """256 distinct lengths over 64 bins, four to a bin, in a scrambled lane order."""
    lengths = (np.arange(256, dtype=np.float32) * np.float32(0.0625))[(np.arange(256) * 37) % 256]
    bins, _, first, count = capi.plan_shadow_regroup(lengths, bins_over_extent=4.0, plan=True)
    assert count == 256 and np.array_equal(bins, (lengths * 4).astype(np.int32))
    assert first.tolist() == [4 * (BINS - 1 - b) for b in range(BINS)]
    check_plan(bins, np.ones(256, bool))


@pytest.mark.parametrize("n", [63, 64, 65, 255])
def test_plan_counts_around_a_wave(n):
    active = np.zeros(256, bool); active[(np.arange(n) * 101) % 256] = True
    assert active.sum() == n
    check_plan((np.arange(256) * 13) % BINS, active)


def test_plan_random_cases():
    rng = np.random.default_rng(11)
    for _ in range(300):
        spread = rng.integers(1, BINS + 1)
        bins = rng.integers(0, spread, 256) + rng.integers(0, BINS + 1 - spread)
        check_plan(bins, rng.random(256) < rng.random())


def test_plan_takes_fewer_lanes_and_refuses_more():
    bins, _, first, count = capi.plan_shadow_regroup([0.3, 5.0, 0.3], bins_over_extent=4.0, plan=True)
    assert bins.tolist() == [1, 20, 1] and count == 3 and first[20] == 0 and first[1] == 1 and first[0] == 3
    with pytest.raises(capi.RestirHipError):
        capi.plan_shadow_regroup(np.zeros(257, np.float32), bins_over_extent=4.0, plan=True)
