"""What the CPU model of the wide bound scan's stage 1 (tests/_wide.py) says, with no GPU: that it is tests/_bound.decide where a wave owns
one tile; that its grid is the library's; that every corpus tests/test_gpu_bound_wide_counts.py pins on the device is what it is built to
be — answered, within the list, loose exactly where it is named loose —; that each of five faults of the form changes a count the device
test compares with ==; and that the planted row of tests/_tight.py stands above 64 results.  No device is touched."""
import numpy as np
import pytest

from tests import _bound as B
from tests import _bound8 as B8
from tests import _oracle as O
from tests import _tight as T
from tests import _wide as Wd
from tests import _widths as W

CUS = 256                                           # an MI355X; the GPU file takes the number from the device and asserts the same conditions


@pytest.mark.parametrize("n,dim", [(6001, 80), (2000, 16)])
def test_one_tile_per_wave_is_the_k64_model(n, dim):
    """tests/test_gpu_bound_scan_wide.py's small corpora at 256 CUs: nothing is dropped, so H, the rows passed on and their count are
    tests/_bound.decide's — with tombstones too, and on the 8-bit intervals"""
    n_tiles = -(-n // 64)
    grid, stride = Wd.plan(n_tiles, CUS)
    assert stride >= n_tiles                                            # one tile per wave
    rows = O.gen_rows(7100 + dim, 0, n, dim)
    q = O.gen_rows(7101 + dim, 0, 1, dim)[0]
    dead = np.ones(n, bool); dead[np.random.default_rng(dim).permutation(n)[:200]] = False
    for metric in (B.COSINE, B.DOT):
        for stage in (B.stage1(metric, B.RowState(rows), q), W.stage8_of(metric, B8.RowState8(rows), q)):
            for live in (np.ones(n, bool), dead):
                for k in (65, 128, 129, 500, 1024):
                    want = B.decide(stage, k, alive=live, cap=Wd.CAP)
                    got = Wd.decide_wide(stage, k, live, n_tiles, grid)
                    assert got["dropped"] == 0 and got["H"] == want["H"] and got["count"] == want["count"], (metric, k, got["count"], want["count"])
                    assert np.array_equal(got["passed"], want["passed"]) and got["hand_back"] == want["hand_back"] and not got["hand_back"]


def test_declined_rows_enter_with_the_librarys_upper_bound():
    """70 rows the bound is sure of at k = 100: the declined rows' keys (the library gives them a NaN upper bound, read here, not assumed)
    sort behind every number, the k-th key is one of theirs and there is no H — as tests/_bound.decide says"""
    n, dim, k = 2000, 16, 100
    rows = O.gen_rows(7600, 0, n, dim)
    bad = np.ones(n, bool); bad[np.random.default_rng(76).permutation(n)[:70]] = False
    rows[bad, 3] = np.nan
    stage = B.stage1(B.COSINE, B.RowState(rows), O.gen_rows(7601, 0, 1, dim)[0])
    assert stage["unsure"].sum() == n - 70 and not np.isfinite(stage["hi"][stage["unsure"]]).any()
    n_tiles = -(-n // 64)
    got = Wd.decide_wide(stage, k, np.ones(n, bool), n_tiles, Wd.plan(n_tiles, CUS)[0])
    assert got["H"] is None and got["hand_back"] and B.decide(stage, k)["H"] is None
    assert Wd.decide_wide(stage, 70, np.ones(n, bool), n_tiles, Wd.plan(n_tiles, CUS)[0])["H"] is not None


@pytest.mark.parametrize("cus", [1, 64, 256, 304])
def test_the_grid_is_the_librarys(cus):
    for rows in (512, 6001, 131_072, 131_073, 200_000, 393_179, 1_000_000, 10_000_000):
        grid, stride = Wd.plan(-(-rows // 64), cus)
        assert stride == 4 * grid
        for dim, k in ((16, 65), (64, 1024)):
            assert Wd.lists_bytes(grid) in Wd.library_regions(dim, rows, k, cus), (cus, rows, grid)
    # what the issue's figures say of 256 CUs: one tile per wave up to 2 048 tiles, two at 200 000 rows with a stride of 1 564
    assert Wd.plan(2048, 256) == (512, 2048) and Wd.plan(3125, 256) == (391, 1564) and Wd.plan(2049, 256)[1] < 2049


def test_the_corpora_are_sized_from_the_compute_units():
    for cus in (64, 256, 304):
        for name, (per, dim, _) in Wd.BASES.items():
            n = Wd.sizes(cus)[per - 2]
            assert Wd.plan(-(-n // 64), cus) == (2 * cus, 8 * cus) and -(-n // 64) == per * 8 * cus and n % 64 != 0
    assert Wd.sizes(256) == (262_107, 393_179)


@pytest.mark.parametrize("name", Wd.CASES)
def test_conditions_of_every_pinned_case(name):
    """answered and within the list; loose exactly where named: keys dropped and MORE survivors than the exact threshold leaves"""
    c = Wd.case(name, CUS)
    for arm in Wd.ARMS:
        for k in c["ks"]:
            m, e = Wd.model(name, CUS, arm, k), Wd.exact_model(name, CUS, arm, k)
            print("%s %s k %d: the model %d (dropped %d), an exact H %d" % (name, arm, k, m["count"], m["dropped"], e["count"]))
            assert not m["hand_back"] and k <= m["count"] <= Wd.CAP, (name, arm, k, m["count"])
            if c["loose"] and k in c["same_count_ks"]:                  # (keys dropped, H looser, and the cluster of near rows is all either H passes)
                assert m["dropped"] > 0 and m["H"] > e["H"] and m["count"] == e["count"] == len(c["at"]), (name, arm, k, m["dropped"], m["count"], e["count"])
            elif c["loose"]:
                assert m["dropped"] > 0 and m["count"] > e["count"], (name, arm, k, m["dropped"], m["count"], e["count"])
            else:
                assert m["dropped"] == 0 and m["count"] == e["count"] and m["H"] == e["H"], (name, arm, k, m["dropped"], m["count"], e["count"])


def test_what_the_loose_cases_drop():
    """one wave holds 128 (192) of the answer and publishes 64; eight waves hold 1 024 and publish 512; with 30 of the 128 removed and 10
    overwritten 88 are left, 64 published; of 70 copies of one row the 64 with the smaller row numbers are kept"""
    for arm in Wd.ARMS:
        assert [Wd.model("loose_one", CUS, arm, k)["dropped"] for k in (65, 100, 129, 500)] == [1, 36, 64, 64]
        assert [Wd.model("loose_one/three", CUS, arm, k)["dropped"] for k in (65, 100, 129, 500)] == [1, 36, 65, 128]
        assert [Wd.model("loose_many/two64", CUS, arm, k)["dropped"] for k in (1024, 500)][0] == 512
        assert [Wd.model("loose_tombstones", CUS, arm, k)["dropped"] for k in (65, 100, 129, 500)] == [1, 24, 24, 24]
        c = Wd.case("loose_ties", CUS)
        m = Wd.model("loose_ties", CUS, arm, 129)
        pub = set((Wd.published(m["lo"], m["hi"], m["unsure"], Wd.live_of(c, CUS), 16 * CUS, 2 * CUS) & np.uint64(0xFFFFFFFF)).tolist())
        assert m["dropped"] == 6 and [int(r) in pub for r in c["at"]] == [True] * 64 + [False] * 6
    c = Wd.case("loose_tombstones", CUS)
    m = Wd.model("loose_tombstones", CUS, "bf16", 129)
    assert not m["passed"][c["removed"]].any() and not m["passed"][c["upd_at"]].any()          # gone, and far away now


@pytest.mark.parametrize("name", Wd.CASES)
def test_every_fault_changes_a_compared_count(name):
    """contiguous blocks of tiles per wave; a list of 63; H one rank too far; dead rows keyed; under a filter, unselected rows keyed: on every
    pinned case and arm at least one k's count moves, so the == of the device test fails for a kernel wrong in one of these ways.  (The
    first two on the loose cases: tests/_wide.faults says why Gaussian rows cannot show them.)"""
    c = Wd.case(name, CUS)
    assert ("blocks" in Wd.faults(name, CUS)) == c["loose"] and ("dead rows keyed" in Wd.faults(name, CUS)) == (c["removed"] is not None)
    assert ("unselected rows keyed" in Wd.faults(name, CUS)) == (c["select"] is not None)
    for arm in Wd.ARMS:
        right = [Wd.model(name, CUS, arm, k)["count"] for k in c["ks"]]
        for fault, args in Wd.faults(name, CUS).items():
            wrong = [Wd.model(name, CUS, arm, k, **args)["count"] for k in c["ks"]]
            assert wrong != right, (name, arm, fault, right)


@pytest.mark.parametrize("metric,dim,k", Wd.PLANTED)
def test_the_planted_row_above_64_results(metric, dim, k):
    """(a) - (d) of tests/_tight.py at k = 65 and 129, (d) against the wide form's list; one tile per wave, so the wide model is the exact one"""
    case = T.planted(metric, dim, k)
    _, _, count = T.conditions(case, cap=Wd.CAP)
    n = len(case["rows"]); n_tiles = -(-n // 64)
    grid, stride = Wd.plan(n_tiles, CUS)
    assert stride >= n_tiles
    m = Wd.decide_wide(B.stage1(metric, B.RowState(case["rows"]), case["q"]), k, np.ones(n, bool), n_tiles, grid)
    assert m["count"] == count and m["dropped"] == 0 and m["passed"][case["target"]] and not m["hand_back"]
