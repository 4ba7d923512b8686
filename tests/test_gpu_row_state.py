"""The per-row state the bound scan's interval rests on, read back from the device (DeviceIndex.debug_read) and compared with a float64
reference: |r| (k_ingest, k_ingest_tiled, k_generate), |r - bf16(r)| rounded up (k_row_residual) and the bfloat16 copy in the layout
stage 1 streams (k_bf16_plane) — after an add, add_synthetic, an add that starts inside a partly filled tile, an add that grows the
arrays, updates in the first, a middle and the last tile, and a remove.  The search tests cannot see this state: the interval's margin
is tens of times wider than the error it covers on their corpora.

The copy's layout is restated HERE from the comment above k_bf16_plane — [tile][16-dim step][32-row block][8-dim half][row of block]
[8 values] — in numpy, independent of the index arithmetic of the writer and of the scan."""
import functools
import os

import numpy as np
import pytest

import quiver_amd
from quiver_amd import _lib
from tests import _bound as B
from tests import _extremes as X
from tests import _oracle as O
from tests._tight import halfway

pytestmark = pytest.mark.gpu

DIMS = (4, 16, 20, 24, 48, 100, 128, 768, 10, 67)          # odd dim4 (20, 100), odd dim8 (24, 100), whole steps; 10 and 67: no multiple of 4 (k_ingest)
N_A, N_S, N_B, N_C = 300, 200, 250, 1500                   # add, add_synthetic, add inside a partly filled tile, add that grows the arrays (16 tiles -> 40)
SEED = 9100


def mixture(rng, n, dim):
    """ordinary rows, rows exact in bfloat16, half-way rows, elements below 2^-126, a whole-denormal and an all-zero row, a row whose
    elements round to bfloat16 infinity, and the extreme classes"""
    rows = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    rows[1::5] = B.bf16(rows[1::5])
    rows[2::5] = halfway(rows[2::5])
    small = rows[3::5]; small[:, ::3] = (small[:, ::3].astype(np.float64) * 1e-41 / 10.0 ** 3).astype(np.float32); small[:, 1] = np.array([0x007FFFFF], np.uint32).view(np.float32)[0]; rows[3::5] = small    # (and one just under 2^-126 whose image rounds UP to it: not flushed)
    rows[4] = (rng.standard_normal(dim) * 1e-39).astype(np.float32)
    rows[9] = 0.0
    rows[14] = np.float32(3.4e38) * np.where(rng.random(dim) < 0.5, -1, 1).astype(np.float32)     # finite, above the largest bfloat16
    rows[19] = -0.0
    for j, (_, _, v) in enumerate(X.class_rows(rng, dim)):
        rows[24 + 5 * j] = v
    return rows


class Expected:
    def __init__(self, rows):
        self.rows = rows
        self.finite = np.isfinite(rows).all(axis=1)
        with np.errstate(all="ignore"):
            self.rn = B.chain_norm_rows(rows)
            self.rh = B.bf16(rows)
            self.rh_bits = (self.rh.view(np.uint32) >> 16).astype(np.uint16)
            self.nan = np.isnan(rows)                                      # (a NaN stays a NaN in the copy, whatever its payload)
            flushed = np.where(np.abs(self.rh) < np.float32(1.17549435e-38), np.float32(0.0), self.rh)      # a subnormal image counts whole
            d = rows.astype(np.float64) - flushed.astype(np.float64)
            self.res64 = np.sqrt(np.sum(d * d, axis=1))
            self.res_up = B.residual_up_rows(rows, flushed)
            self.res_top = np.nextafter(self.res_up, np.float32(np.inf))
            self.exact = self.finite & (rows.view(np.uint32) & 0xFFFF == 0).all(axis=1) & ~(np.abs(self.rh) < np.float32(1.17549435e-38)).any(axis=1) | \
                (self.finite & (rows == 0).all(axis=1))


@functools.lru_cache(maxsize=None)
def corpus(dim):
    """the rows every step of the sequence adds, and what the reference derives from them: computed once per dimension, never written to"""
    rng = np.random.default_rng(31 * dim + 1)
    parts = [mixture(rng, N_A, dim), O.gen_rows(SEED + dim, 0, N_S, dim), mixture(rng, N_B, dim), mixture(rng, N_C, dim)]
    rows = np.concatenate(parts)
    n = len(rows)
    assert 1000 <= n <= 5000 and n % 64 and (N_A + N_S) % 64
    assert (N_A + N_S + N_B) <= max(16, -(-N_A // 64)) * 64 < n                           # the first add reserves max(need, 16) tiles: three adds fit, the fourth grows the arrays
    new = mixture(np.random.default_rng(31 * dim + 2), 130, dim)[[0, 1, 2]]            # ordinary, exact in bfloat16, half-way
    rows.setflags(write=False)
    return rows, Expected(rows), new, Expected(new)


def decode(plane, tiles, dim):
    """[tiles * 64, steps * 16] uint16 from [tile][step][block of 32 rows][half of 8 dims][row of the block][8 values]"""
    steps = (dim + 15) // 16
    return plane.reshape(tiles, steps, 2, 2, 32, 8).transpose(0, 2, 4, 1, 3, 5).reshape(tiles * 64, steps * 16)


def read_state(idx, n):
    tiles = (n + 63) // 64
    rn, rr, pl = idx.debug_read("rnorm"), idx.debug_read("rres"), idx.debug_read("plane")
    assert rn.size == tiles * 64 and rr.size == tiles * 64
    return rn[:n], rr[:n], decode(pl, tiles, idx.dim)[:n, :idx.dim]


def same64(got, want):
    nw = np.isnan(want)
    return np.array_equal(np.isnan(got), nw) and np.array_equal(got[~nw].view(np.uint64), want[~nw].view(np.uint64))


def check(idx, exp, n, live, what):
    """every live row of the first n against the reference"""
    rn, rr, pl = read_state(idx, n)
    live = live[:n]
    e_rn, fin = exp.rn[:n][live], exp.finite[:n][live]
    assert same64(rn[live], e_rn), (what, "rnorm", np.flatnonzero(live)[~((rn[live] == e_rn) | (np.isnan(rn[live]) & np.isnan(e_rn)))][:5])
    g = rr[live][fin].astype(np.float64)
    with np.errstate(all="ignore"):
        low = g >= exp.res64[:n][live][fin]
        high = rr[live][fin] <= exp.res_top[:n][live][fin]
    rows_at = np.flatnonzero(live)[fin]
    assert low.all(), (what, "rres below the float64 residual", rows_at[~low][:5], g[~low][:5], exp.res64[:n][live][fin][~low][:5])
    assert high.all(), (what, "rres above residual_up plus one step", rows_at[~high][:5], g[~high][:5], exp.res_top[:n][live][fin][~high][:5])
    ex = exp.exact[:n] & live
    assert ex.sum() >= 3 and not rr[ex].any(), (what, "rres of rows exact in bfloat16", np.flatnonzero(ex)[rr[ex] != 0][:5])
    want = exp.rh_bits[:n][live]; got = pl[live]
    nan = exp.nan[:n][live]
    isnan16 = ((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)
    ok = np.where(nan, isnan16, got == want)
    assert ok.all(), (what, "the bfloat16 copy: (row, dim) %s got %s want %s" % (
        [(int(np.flatnonzero(live)[i]), int(j)) for i, j in np.argwhere(~ok)[:5]], got[~ok][:5], want[~ok][:5]))
    return rn, rr, pl


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("dim", DIMS)
def test_row_state_follows_every_write(metric, dim):
    rows, exp, new, exp_new = corpus(dim)
    n = len(rows)
    idx = quiver_amd.DeviceIndex(dim, metric, bf16_rows=metric == "l2")    # (an l2 index keeps the copy only when asked to)
    live = np.ones(n, bool)
    a, s, b = N_A, N_A + N_S, N_A + N_S + N_B
    idx.add(rows[:a]); check(idx, exp, a, live, "add")
    idx.add_synthetic(SEED + dim, 0, N_S); check(idx, exp, s, live, "add_synthetic")
    assert np.array_equal(idx.get_rows(np.arange(a, s)).view(np.uint32), rows[a:s].view(np.uint32))
    idx.add(rows[s:b]); before = check(idx, exp, b, live, "add inside a partly filled tile")
    idx.add(rows[b:]); after = check(idx, exp, n, live, "add that grows the arrays")
    assert same64(after[0][:b], before[0]) and X.same(after[1][:b], before[1]) and np.array_equal(after[2][:b], before[2]), "rows from before the growth"

    # updates in the first, a middle and the last tile: the state is the NEW row's
    cur = rows.copy(); cur_exp = Expected(cur)                             # (a copy: the shared reference stays as it is)
    old_rr = after[1]
    for j, at in enumerate((5, (n // 128) * 64 + 37, n - 2)):
        assert exp.finite[at] and exp.res_up[at] != exp_new.res_up[j]      # old and new residual differ: a stale one cannot pass
        idx.update(at, new[j]); cur[at] = new[j]
        for name in ("finite", "nan", "rn", "rh_bits", "res64", "res_up", "res_top", "exact"):
            getattr(cur_exp, name)[at] = getattr(exp_new, name)[j]
    rn, rr, pl = check(idx, cur_exp, n, live, "update")
    for j, at in enumerate((5, (n // 128) * 64 + 37, n - 2)):
        assert rr[at] != old_rr[at] and exp_new.res64[j] <= rr[at] <= exp_new.res_top[j]

    gone = np.unique(np.concatenate([np.arange(64, 130), [0, 7, n - 1]]))
    idx.remove(gone.astype(np.uint32)); live[gone] = False
    check(idx, cur_exp, n, live, "remove")
    idx.close()


def test_arrays_the_index_does_not_keep_and_short_buffers():
    rows = O.gen_rows(78, 0, 1000, 128)
    for make in ("flag", "oom", "l2"):
        if make == "oom":
            os.environ["QV_TEST_PLANE_OOM"] = "1"                          # the copy's allocation answers out-of-memory: not an error, no copy
        try:
            idx = quiver_amd.DeviceIndex(128, "l2" if make == "l2" else "cosine", scan_plane=make != "flag")
            idx.add(rows)
        finally:
            os.environ.pop("QV_TEST_PLANE_OOM", None)
        with pytest.raises(quiver_amd.QvError) as e:
            idx.debug_read("plane")
        assert e.value.code == _lib.QV_ERR_UNSUPPORTED, make
        assert same64(idx.debug_read("rnorm")[:1000], B.chain_norm_rows(rows))
        assert idx.debug_read("rres").size == 1024
        idx.close()
    idx = quiver_amd.DeviceIndex(128, "l1"); idx.add(rows)                 # a metric whose ingest derives nothing
    for what in ("rnorm", "rres", "plane"):
        with pytest.raises(quiver_amd.QvError) as e:
            idx.debug_read(what)
        assert e.value.code == _lib.QV_ERR_UNSUPPORTED, what
    idx.close()
    idx = quiver_amd.DeviceIndex(128, "cosine"); idx.add(rows)
    out = np.empty(1024, np.float64)
    assert _lib.lib().qv_index_debug_read(idx.handle, 0, out.ctypes.data, out.nbytes - 1) == _lib.QV_ERR_INVALID_ARG
    assert _lib.lib().qv_index_debug_read(idx.handle, 3, out.ctypes.data, out.nbytes) == _lib.QV_ERR_INVALID_ARG
    assert _lib.lib().qv_index_debug_read(idx.handle, 0, out.ctypes.data, out.nbytes) == _lib.QV_OK
    idx.close()
