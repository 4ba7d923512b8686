"""Which kernels answer a fused flat search (k <= 64), restated in Python from DESIGN.md 4.1's priority order — the expectation that
tests/test_flat_route_cpu.py holds the library's own decision (quiver_amd/csrc/qv_scan.hip: plan_flat, through qv_scan_route) against,
and the route names tests/test_gpu_flat_route.py looks its cases up by.

The three bound rules are asked through their exports (qv_scan_bound_applies, qv_scan_bound_applies_filtered, qv_scan_bound8_applies:
tests/test_bound_scan*_cpu.py check those); everything else — the workgroup count, the small-collection rule, the two tile-over-eight-
waves rules, the matrix-core scan's conditions — is restated here from its definition, with the default environment knobs."""
import functools

import quiver_amd
from quiver_amd import _lib

ROUTES = ("small", "bound_mq", "split_mq", "mq64", "mq", "bound", "bound8_first", "split", "fused", "two_launch")
SMALL, BOUND_MQ, SPLIT_MQ, MQ64, MQ, BOUND, BOUND8_FIRST, SPLIT, FUSED, TWO_LAUNCH = range(10)
BOUND_ROUTES = (BOUND_MQ, BOUND, BOUND8_FIRST)
NO_FILTER = 0xFFFFFFFF
AUTO, ALWAYS, NEVER = 0, 1, 2
CUS = 256                                                    # an MI355X

M = {name: quiver_amd.metric_id(name) for name in ("cosine", "l2", "l2sq", "dot", "l1", "cosine_f32", "l2_f32", "dot_f32", "l2sq_f64")}
_SPLIT_METRICS = (M["cosine"], M["dot"], M["l2"], M["l1"], M["l2sq_f64"])
_F64_QUERY = (M["cosine"], M["dot"], M["l2sq_f64"])           # metrics whose query is staged as float64


def library_route(metric, dim, rows, nq, k, tickets, bound_mode, plane_mode, has_plane, has_plane8, candidate_tiles, cus=CUS):
    return _lib.lib().qv_scan_route(metric, dim, rows, nq, k, cus, tickets, bound_mode, plane_mode, has_plane, has_plane8, candidate_tiles)


@functools.lru_cache(maxsize=None)
def bound_rule(metric, dim, rows, nq, k, mode, has_plane, candidate_tiles):
    """the bound rule that takes the call: the filtered one when candidate_tiles is not NO_FILTER"""
    if candidate_tiles == NO_FILTER:
        rc = _lib.lib().qv_scan_bound_applies(metric, dim, rows, nq, k, mode, has_plane)
    else:
        rc = _lib.lib().qv_scan_bound_applies_filtered(metric, dim, rows, nq, k, mode, has_plane, candidate_tiles)
    assert rc in (0, 1), rc
    return bool(rc)


@functools.lru_cache(maxsize=None)
def bound8_rule(metric, dim, rows, nq, k, mode, plane_mode, has_plane8):
    rc = _lib.lib().qv_scan_bound8_applies(metric, dim, rows, nq, k, mode, plane_mode, has_plane8)
    assert rc in (0, 1), rc
    return bool(rc)


def scan_grid(n_tiles, cus=CUS):
    """plan_scan: one tile per wave at most, two workgroups of four waves per CU, short shares evened out"""
    want = (n_tiles + 3) // 4
    cap = cus * 2
    grid = max(1, min(want, cap))
    if want > cap:
        waves = grid * 4
        per = (n_tiles + waves - 1) // waves
        need = (n_tiles + per - 1) // per
        if per <= 32:
            grid = (need + 3) // 4
    return grid


def _query_lds(metric, dim4):
    return (dim4 * 4 * (8 if metric in _F64_QUERY else 4) + 15) // 16 * 16


def flat_small_applies(n_tiles, nq, k):
    return n_tiles <= 256 and 1 <= nq <= 4 and 1 <= k <= 16


def flat_split_applies(metric, dim4, n_tiles, nq, k):
    lds = _query_lds(metric, dim4) + 3 * 8 * 64 * 8 + 40 * 1024
    return metric in _SPLIT_METRICS and nq == 1 and 1 <= k <= 64 and dim4 >= 32 and lds <= 160 * 1024 and 2 <= n_tiles <= 2560


def flat_split_mq_applies(metric, dim4, n_tiles, nq, k):
    qb = 4 if nq <= 4 else 8
    lds = qb * dim4 * 4 * (8 if metric in _F64_QUERY else 4) + qb * 8 * 64 * 8 + 1024
    reads = ((nq + qb - 1) // qb) * n_tiles * dim4 * 1024
    return (metric in _SPLIT_METRICS and 2 <= nq <= 32 and 1 <= k <= 64 and dim4 >= 16 and lds <= 160 * 1024 and 2 <= n_tiles <= 2560
            and reads <= 600 * 1000 * 1000)


def mq64_applies(metric, dim4, nq):
    """the f64 matrix-core scan's own conditions (mq64_blocks != 0): cosine or dot, and the shape's LDS fits a CU"""
    if metric not in (M["cosine"], M["dot"]):
        return False
    h, nb, w, wgs = (1, 1, 4, 2) if nq <= 16 else (1, 2, 8, 1)
    lds = max(h * nb * dim4 * 64 * 4 + h * w * 4 * 64 * 8, h * (w - 1) * 16 * nb * 64 * 8)
    return lds * wgs <= 158 * 1024


def shared_pass(metric, dim4, n_tiles, grid, n, k):
    """n queries that carry no tickets: steps 3, 4 and 8 -> (route, queries per corpus pass)"""
    if n < 2:
        return TWO_LAUNCH, 0
    if flat_split_mq_applies(metric, dim4, n_tiles, n, k):
        return SPLIT_MQ, 4 if n <= 4 else 8
    if n >= 9 and n_tiles >= 16 * grid and mq64_applies(metric, dim4, n):
        return MQ64, 0
    f32_acc = metric in (M["l2sq"], M["cosine_f32"], M["l2_f32"], M["dot_f32"])
    return MQ, (8 if f32_acc else 16) if n >= 9 else (8 if n >= 5 else 4)


def expected_plan(metric, dim, rows, nq, k, tickets, bound_mode, plane_mode, has_plane, has_plane8, candidate_tiles, cus=CUS):
    """-> (route, qb, remainder queries, remainder's route, remainder's qb)"""
    dim4, n_tiles = (dim + 3) // 4, (rows + 63) // 64
    grid = scan_grid(n_tiles, cus)
    filtered = candidate_tiles != NO_FILTER
    takes = bool(tickets) and bound_rule(metric, dim, rows, nq, k, bound_mode, has_plane, candidate_tiles)
    # 1. small (with the default knobs "the bound rule declines" and "no bound route" are the same calls)
    if not takes and tickets and flat_small_applies(n_tiles, nq, k) and not flat_split_applies(metric, dim4, n_tiles, nq, k):
        return SMALL, 0, 0, TWO_LAUNCH, 0
    if nq >= 2:
        # 2. bound_mq
        if takes and (bound_mode == ALWAYS or not flat_split_mq_applies(metric, dim4, n_tiles, nq, k)):
            return BOUND_MQ, 4 if nq <= 4 else 8, 0, TWO_LAUNCH, 0
        # 3. / 4.
        route, qb = shared_pass(metric, dim4, n_tiles, grid, nq, k)
        rem = nq & 31
        if route == MQ64 and nq > 32 and 1 <= rem <= 8:
            route, qb = shared_pass(metric, dim4, n_tiles, grid, nq - rem, k)
            return (route, qb, rem) + shared_pass(metric, dim4, n_tiles, grid, rem, k)
        return route, qb, 0, TWO_LAUNCH, 0
    # 5. bound / bound8_first
    if takes and grid > 1:
        first8 = not filtered and bool(has_plane) and bound8_rule(metric, dim, rows, nq, k, bound_mode, plane_mode, has_plane8)
        return BOUND8_FIRST if first8 else BOUND, 0, 0, TWO_LAUNCH, 0
    # 6. split  7. fused  8. two_launch
    if tickets and flat_split_applies(metric, dim4, n_tiles, nq, k):
        return SPLIT, 0, 0, TWO_LAUNCH, 0
    if tickets and grid > 1:
        return FUSED, 0, 0, TWO_LAUNCH, 0
    return TWO_LAUNCH, 0, 0, TWO_LAUNCH, 0


def expected_route(*args, **kw):
    return expected_plan(*args, **kw)[0]
