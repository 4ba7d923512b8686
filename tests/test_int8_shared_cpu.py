"""Which of the int8 filter's two kernels a batch takes (qv_batched_int8_form): 0 none — exactly where qv_batched_int8_applies is 0 —, 1 the block
kernel, 2 the shared-row kernel on the call's first piece.  The automatic mode's cells are the ones profiles/LAB_r31_int8_shared.md measured."""
import pytest

import quiver_amd
from quiver_amd import _lib

M = 1_000_000


@pytest.mark.parametrize("metric,dim,rows,nq,k,filt,plane8,mode,want", [
    ("cosine", 768, M, 256, 10, "int8", True, "shared", 2),
    ("dot_product", 128, M, 129, 10, "int8", True, "shared", 2),      # one query past two blocks: padded to a whole group
    ("cosine", 384, M, 256, 64, "int8", True, "shared", 2),
    ("dot_product", 512, M, 1024, 100, "int8", True, "shared", 2),
    ("cosine", 768, M, 300, 10, "int8", True, "shared", 2),           # 256 on the shared-row kernel (then 44 on the block kernel)
    ("cosine", 768, M, 256, 10, "int8", True, "blocks", 1),
    ("dot_product", 128, M, 129, 10, "int8", True, "blocks", 1),
    ("cosine", 768, M, 128, 10, "int8", True, "shared", 1),           # no whole group
    ("cosine", 768, M, 64, 10, "int8", True, "shared", 1),
    ("cosine", 96, M, 256, 10, "int8", True, "shared", 1),            # dimensions without an instantiation
    ("cosine", 1024, M, 256, 10, "int8", True, "shared", 1),
    ("euclidean", 768, M, 256, 10, "int8", True, "shared", 0),        # wherever no int8 kernel runs
    ("cosine", 768, M, 256, 10, "int8", False, "shared", 0),
    ("cosine", 768, M, 256, 10, "auto", True, "shared", 0),
    ("cosine", 768, M, 8, 10, "int8", True, "shared", 0),
    # the automatic mode, LAB r31's table: ahead by more than both arms' spread at 10M x 768 (129, 256, 1024 queries; k = 10 and 64) ...
    ("cosine", 768, 10 * M, 129, 10, "int8", True, "auto", 2),
    ("cosine", 768, 10 * M, 256, 10, "int8", True, "auto", 2),
    ("cosine", 768, 10 * M, 256, 64, "int8", True, "auto", 2),
    ("cosine", 768, 10 * M, 1024, 10, "int8", True, "auto", 2),
    # ... the ranges overlap at 1M x 768 and at 10M x 128; dot, 384 / 512 dimensions and the corpora between were not measured
    ("cosine", 768, M, 129, 10, "int8", True, "auto", 1),
    ("cosine", 768, M, 256, 10, "int8", True, "auto", 1),
    ("cosine", 768, M, 256, 64, "int8", True, "auto", 1),
    ("cosine", 768, M, 1024, 10, "int8", True, "auto", 1),
    ("cosine", 128, 10 * M, 256, 10, "int8", True, "auto", 1),
    ("cosine", 768, 5 * M, 256, 10, "int8", True, "auto", 1),
    ("dot_product", 768, 10 * M, 256, 10, "int8", True, "auto", 1),
    ("cosine", 512, 10 * M, 256, 10, "int8", True, "auto", 1),
])
def test_form(metric, dim, rows, nq, k, filt, plane8, mode, want):
    assert quiver_amd.batched_int8_form(metric, dim, rows, nq, k, filter=filt, has_plane8=plane8, mode=mode) == want
    assert (want != 0) is quiver_amd.batched_int8_applies(metric, dim, rows, nq, k, filter=filt, has_plane8=plane8)


@pytest.mark.parametrize("mode", [-1, 3])
def test_bad_mode(mode):
    assert _lib.lib().qv_batched_int8_form(0, 768, M, 256, 10, 5, 1, mode) < 0
