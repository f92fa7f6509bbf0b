"""The model of the meter ranks (tests/meter_rank_model.py) and the coverage of its data, without a GPU: the scenes and the k values
the stand-in and the GPU tests run are checked HERE to reach every digit of the kernel's radix select, the ties across a wavefront
and a chunk boundary, and the corner counts - so that a kernel that passes those tests has been asked every one of these.

The rows are those of a program whose output is its input, computed by the numpy models of the meters (route_models.meter_model,
meter_target_model.match_model, meter_level_model.level_model)."""
import os
import re

import numpy as np

import meter_level_model as L
import meter_list_model as M
import meter_rank_model as R
import meter_target_model as T
from route_models import meter_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_digit_width_is_the_kernels():
    hpp = open(os.path.join(ROOT, "fx8010-emulator-core_amd", "csrc", "fx_meter_rank.hpp")).read()
    assert int(re.search(r"constexpr int kMeterRankDigitBits = (\d+);", hpp).group(1)) == R.DIGIT_BITS
    assert R.PASSES * R.DIGIT_BITS == 64
    header = open(os.path.join(ROOT, "include", "fx8010_amd.h")).read()
    assert re.search(r"#define FXB_METER_LARGEST \(1u << 1\)", header) and R.LARGEST == 2 and R.BELOW == 1
    for family in R.FAMILIES:
        assert re.search(r"int64_t %s\(fxb_handle\* h, int stat, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t\* list, double\* value, unsigned flags\);" % R.CALL[family], header)
    for name, number in (("FXB_INFO_METER_RANKS", 71), ("FXB_INFO_METER_MATCH_RANKS", 72), ("FXB_INFO_METER_LEVEL_RANKS", 73)):
        assert re.search(r"%s = %d\b" % (name, number), header), name


def test_the_keys_are_monotone_in_the_real_order():
    v = np.array([-np.inf, -1e300, -1.0, -1e-310, -0.0, 0.0, 5e-324, 1e-310, 1.0, 1.0 + 2.0 ** -52, 2.0, 1e300, np.inf])
    k = R.keys(v)
    assert k[4] == k[5], "-0.0 and +0.0 have one key"
    rest = np.delete(k, 4)
    assert (rest[1:] > rest[:-1]).all() and (R.keys(np.delete(v, 4), largest=True)[1:] < R.keys(np.delete(v, 4), largest=True)[:-1]).all()
    assert R.first_digit(R.keys(np.array([1.0]))[0], R.keys(np.array([1.0 + 2.0 ** -52]))[0]) == R.PASSES - 1
    assert R.first_digit(R.keys(np.array([-1.0]))[0], R.keys(np.array([1.0]))[0]) == 0 and R.first_digit(k[4], k[5]) is None


def test_rank_is_the_sorted_selection():
    rng = np.random.default_rng(1)
    V = rng.integers(-3, 4, 500).astype(np.float64)
    V[7] = -0.0
    for below in (False, True):
        for largest in (False, True):
            for first, n_range, t in ((0, 500, -np.inf), (0, 500, 1.0), (37, 300, 0.0), (499, 1, 0.0), (5, 0, 0.0)):
                cand = [n for n in range(first, first + n_range) if (V[n] < t if below else V[n] >= t)]
                want = sorted(cand, key=lambda n: (-V[n] if largest else V[n], n))
                for k in (0, 1, 5, len(want), len(want) + 3):
                    m, lst, val = R.rank(V, k, t, below, largest, first, n_range)
                    assert m == len(cand) and lst.tolist() == want[:k] and np.array_equal(val.view(np.uint64), V[want[:k]].view(np.uint64))


def ladder_rows():
    return meter_model(R.ladder_voices())


def test_the_ladder_reaches_every_digit_below_the_top_one_and_the_target_scene_the_top():
    rows = ladder_rows()
    energy = R.value("meter", rows, 0)
    assert sorted(np.unique(energy).tolist()) == sorted([0.25, 1.0] + [1.0 + 2.0 ** (-2 * j) for j in R.LADDER_J]), "the sums are exact"
    assert (energy == 1.0).sum() == R.LADDER_N - len(R.LADDER_HALF) - len(R.LADDER_AT) == 288
    seen = set(R.digit_ks(energy)) | set(R.digit_ks(energy, largest=True))
    assert seen >= set(range(1, R.PASSES)), seen
    ones = len(R.LADDER_HALF) + 288
    assert R.digit_ks(energy)[R.PASSES - 1] == ones, "1.0 against 1.0 + 2^-52: the lowest digit"
    assert R.first_digit(*R.keys(np.array([1.0, 1.0 + 2.0 ** -52]))) == R.PASSES - 1
    # the top digit: a negative against a positive cross
    x = M.voices(200, 1, 33, seed=1)
    match, _ = T.match_model(x, R.target_for(x), 1, 0, False)
    cross = R.value("match", match, T.CROSS)
    assert (cross < 0).sum() > 10 and (cross > 0).sum() > 10 and (cross == 0).any()
    k = R.digit_ks(cross)[0]
    assert k == (cross < 0).sum(), "the k-th key is the largest negative cross, the next one is not negative"
    assert seen | set(R.digit_ks(cross)) >= set(range(R.PASSES))


def test_the_ladder_has_ties_at_the_kth_key_across_a_wavefront_and_a_chunk_boundary():
    energy = R.value("meter", ladder_rows(), 0)
    for k, border in ((100, R.WAVE), (270, R.CHUNK)):
        equals, take = R.tie(energy, k)
        winners = equals[:take]
        assert 0 < take < equals.size, "fewer of the equals win than exist"
        assert winners.min() < border <= winners.max() and (np.diff(equals) == 1).sum() > take // 2, (k, border)
        m, lst, _ = R.rank(energy, k)
        assert m == R.LADDER_N and set(winners.tolist()) <= set(lst.tolist()) and equals[take] not in lst
    # LARGEST with ties: the peaks are 1.0 (295 voices) and 0.5
    peak = R.value("meter", ladder_rows(), 1)
    equals, take = R.tie(peak, 100, largest=True)
    assert equals.size == 295 and take == 100 and R.rank(peak, 100, largest=True)[1].tolist() == equals[:100].tolist()


def test_the_corner_counts_are_among_the_cases():
    rows = ladder_rows()
    energy = R.value("meter", rows, 0)
    t = 1.0 + 2.0 ** -30
    m = R.rank(energy, 0, t)[0]
    assert m == 4 and {m - 1, m, m + 1, 0} <= set(R.k_values(m)), "M < k, M == k, k == 0 on a threshold inside the ladder"
    assert R.rank(energy, 5, t)[1].size == 4 and R.rank(energy, 4, t)[1].size == 4 and R.rank(energy, 0, t)[1].size == 0
    assert R.rank(energy, 3, np.inf)[0] == 0 and np.inf in R.thresholds(energy), "M == 0"
    nonfinite = R.value("meter", rows, 3)
    assert (nonfinite == 0).all() and R.rank(nonfinite, 5)[1].tolist() == [0, 1, 2, 3, 4], "every V equal: the smallest numbers win"
    assert R.rank(nonfinite, 5, largest=True)[1].tolist() == [0, 1, 2, 3, 4]
    assert {63, 64, 65, 257} <= set(R.k_values(300))
    # the level scene: envelopes of several kinds, quiet runs of silent voices
    x = M.voices(200, 2, 33, seed=2)
    level = L.level_model(x, R.LEVEL_RELEASE, R.LEVEL_FLOOR)
    assert np.unique(R.value("level", level, L.ENVELOPE)).size > 4 and np.unique(R.value("level", level, L.QUIET)).size >= 2
