"""CPU: the partial-record layout that AttnTail / AttnHead reduce (train_ops.tail_regions / head_regions) against the
record the built library declares (pcr_attn_tail_part_floats / pcr_attn_head_part_floats, TailShape / HeadShape ::REC of
csrc/train_chain_kernels.hip) for every fused shape: fields disjoint, rows inside their leading dimension, the last
field closing the record -- and the check each backward makes before its launch refuses a record that does not fit."""
import itertools

import pytest

TAIL_SHAPES = [(32, 32, 64, 32), (64, 64, 128, 64), (64, 64, 128, 128), (64, 32, 128, 64), (64, 3, 128, 32)]   # d, c1, hid, out
HEAD_SHAPES = [(32, 32, 32, 3, 7), (64, 64, 64, 3, 7), (64, 64, 64, 2, 2), (128, 64, 64, 2, 2), (64, 64, 64, 3, 4)]  # C, hd, d, n, src


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def _c32(n):
    return (n + 31) // 32 * 32


def _check_layout(regions, rec):
    spans = [(off, off + rows * ld) for off, rows, _, ld in regions]
    assert all(0 <= a < b for a, b in spans)
    for (a0, a1), (b0, b1) in itertools.combinations(spans, 2):
        assert a1 <= b0 or b1 <= a0, "fields overlap: [%d, %d) and [%d, %d)" % (a0, a1, b0, b1)
    assert all(1 <= cols <= ld for _, _, cols, ld in regions)
    assert max(b for _, b in spans) == rec


def test_train_ops_imports_without_a_device():
    import pcr_amd.train_ops as TO
    assert TO.pack_dev is not None and TO._PREPACKS is not None and TO.prepack is not None


@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_regions_tile_the_library_record(lib, shape):
    from pcr_amd import train_ops as TO
    d, c1, hid, out = shape
    regions, rec = TO.tail_regions(*shape), lib.pcr_attn_tail_part_floats(*shape)
    assert rec > 0 and len(regions) == 7
    _check_layout(regions, rec)
    assert regions[1][1:] == (hid, c1 + d, _c32(c1 + d))
    TO.check_part_regions(regions, rec, "tail")


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_regions_tile_the_library_record(lib, shape):
    from pcr_amd import train_ops as TO
    C, hd, d, n, src = shape
    regions, rec = TO.head_regions(C, hd, d, n), lib.pcr_attn_head_part_floats(*shape)
    assert rec > 0 and len(regions) == 4 + n
    _check_layout(regions, rec)
    assert regions[0] == (0, hd, 3, 32)
    TO.check_part_regions(regions, rec, "head")


def test_a_record_that_does_not_fit_is_refused(lib):
    from pcr_amd import _lib as L
    from pcr_amd import train_ops as TO
    tail, head = (48, 32, 64, 32), (48, 32, 32, 3, 7)               # shapes with no fused instantiation: no record
    assert lib.pcr_attn_tail_part_floats(*tail) == 0 and lib.pcr_attn_head_part_floats(*head) == 0
    with pytest.raises(L.PcrError, match="partial record"):
        TO.check_part_regions(TO.tail_regions(*tail), 0, "tail")
    with pytest.raises(L.PcrError, match="partial record"):
        TO.check_part_regions(TO.head_regions(*head[:4]), 0, "head")
    regions = TO.tail_regions(*TAIL_SHAPES[0])                      # ... nor one that is a field longer or shorter
    rec = lib.pcr_attn_tail_part_floats(*TAIL_SHAPES[0])
    for wrong in (rec + TAIL_SHAPES[0][3], rec - TAIL_SHAPES[0][3]):
        with pytest.raises(L.PcrError, match="partial record"):
            TO.check_part_regions(regions, wrong, "tail")
