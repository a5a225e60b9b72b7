"""CPU: tests/farview.py is not vacuous, at reaches small enough for host memory -- the view keeps its values, alignment and
stride rule; rows lie on both sides of every threshold; a store at a WRAPPED offset (the row offset truncated to the
threshold's width, what a 32-bit offset does at the real reaches) is reported with its place; the chunked check sees every
byte of the parent at any chunk size and leaves the logical elements as they were."""
import pytest
import torch

import farview as FV
import redzone as RZ

SMALL = (1 << 14, 1 << 15, 1 << 16)          # stand-ins for 2^31, 2^32 and 2^33 bytes


def _values(rows, cols, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g) if dtype == torch.float32 else torch.randint(0, 100, (rows, cols), generator=g).to(dtype)


def _far(t, reach, fill=RZ.POISON):
    return FV.far(t, reach, fill, device="cpu", thresholds=SMALL)


@pytest.mark.parametrize("fill", [RZ.ZERO, RZ.POISON])
@pytest.mark.parametrize("reach", SMALL)
@pytest.mark.parametrize("rows,cols,dtype", [(5, 64, torch.float32), (70, 12, torch.float32), (3, 8, torch.int32), (7, 16, torch.uint8)])
def test_far_keeps_values_alignment_stride_rule_and_fill(rows, cols, dtype, reach, fill):
    t = _values(rows, cols, dtype)
    v = _far(t, reach, fill)
    f = v._far
    assert torch.equal(v, t) and v.dtype == dtype and v.stride() == (f.ld, 1)
    assert v.data_ptr() % RZ.ALIGN == 0 and f.ld % 4 == 0
    assert FV.farthest(v) > reach and FV.farthest(v) - reach <= 16 * rows * t.element_size() + 64   # just past it
    offs = [r * f.ld * f.isz for r in range(rows)]
    for th in SMALL:
        if th <= reach:
            assert min(offs) < th <= max(offs)
    assert v.data_ptr() - f.parent.data_ptr() >= RZ.MARGIN
    assert f.parent.numel() - (f.off + offs[-1] + cols * f.isz) >= RZ.MARGIN
    assert int((f.parent != fill).sum()) <= t.numel() * t.element_size()
    FV.check_untouched(v)


def test_real_reaches_need_no_memory_to_plan():
    """ld_for at the three real reaches: multiples of 4 that fit an int, rows on both sides, distinct offsets modulo 2^32."""
    for rows in (5, 7, 70, 130):
        for reach in FV.REACHES.values():
            ld = FV.ld_for(rows, reach)
            offs = [r * ld * 4 for r in range(rows)]
            assert ld % 4 == 0 and ld < 2 ** 31 and reach < offs[-1] <= reach + 16 * rows + 64
            assert len({o % 2 ** 32 for o in offs}) == rows
            for th in FV.REACHES.values():
                if th <= reach:
                    assert offs[0] < th <= offs[-1]


@pytest.mark.parametrize("fill", [RZ.ZERO, RZ.POISON])
@pytest.mark.parametrize("th", SMALL)
def test_a_store_at_a_wrapped_offset_is_reported(th, fill):
    """The deliberate wrong write: the last row's first element stored at its byte offset modulo the threshold."""
    t = _values(5, 8, seed=1)
    v = _far(t, th, fill)
    f = v._far
    FV.check_untouched(v)
    wrapped = FV.farthest(v) % th
    assert 0 < wrapped < f.ld * f.isz                                  # (inside row 0's stride: its data or its gap)
    flat = f.parent[f.off:].view(torch.float32)
    before = flat[wrapped // 4 + 8].clone()
    flat[wrapped // 4 + 8] = 7.0                                       # past row 0's 8 columns: the ld gap
    with pytest.raises(AssertionError, match=r"in the ld gap: row 0, column %d " % (wrapped // 4 + 8)):
        FV.check_untouched(v, "wrapped store")
    assert torch.equal(v, t)                                           # the check put the logical elements back
    flat[wrapped // 4 + 8] = before
    FV.check_untouched(v)


@pytest.mark.parametrize("chunk", [8, 64, 4096, FV.CHUNK])
def test_chunked_check_sees_every_region_at_any_chunk_size(chunk):
    t = _values(7, 12, seed=2)
    for where in ("front", "gap", "last gap", "behind", "end"):
        v = _far(t, SMALL[1], RZ.POISON)
        f = v._far
        at = {"front": f.off - 1, "gap": f.off + 12 * 4, "last gap": f.off + 5 * f.ld * 4 + 12 * 4 + 3,
              "behind": f.off + FV.farthest(v) + 12 * 4, "end": f.parent.numel() - 1}[where]
        FV.check_untouched(v, chunk=chunk)
        f.parent[at] = 0x5A
        with pytest.raises(AssertionError, match="byte 0x5a"):
            FV.check_untouched(v, chunk=chunk)
        assert torch.equal(v, t)
        v[3, 5] = 9.0                                                  # stores inside the view are not damage
        f.parent[at] = RZ.POISON
        FV.check_untouched(v, chunk=chunk)


def test_far_rows_places_sparse_rows_and_its_check_sees_the_space_between_them():
    t = _values(6, 8, seed=3)
    at = [0, 3, 500, 501, 1500, 2047]
    v = FV.far_rows(t, at, 8, RZ.POISON, device="cpu")
    f = v._far
    assert v.shape == (2048, 8) and v.stride() == (8, 1) and v.data_ptr() % RZ.ALIGN == 0 and torch.equal(v[at], t)
    assert FV.farthest(v) == 2047 * 8 * 4 and int((f.parent != RZ.POISON).sum()) <= t.numel() * 4
    for chunk in (8, 4096, FV.CHUNK):
        FV.check_untouched(v, chunk=chunk)
        v[502, 0] = 1.0                                                # a row nobody was given: the first one behind logical row 3
        with pytest.raises(AssertionError, match="between the logical rows: 32 bytes past the start of logical row 3"):
            FV.check_untouched(v, chunk=chunk)
        v[502, :1].view(torch.uint8).fill_(RZ.POISON)
        v[1500, 7] = 2.0                                               # inside a logical row: not damage
        FV.check_untouched(v, chunk=chunk)
    with pytest.raises(ValueError):
        FV.far_rows(t, at[:5], 8, device="cpu")


def test_far_refuses_what_it_cannot_lay_out():
    with pytest.raises(ValueError):
        FV.far(torch.zeros(1, 8), SMALL[0], device="cpu", thresholds=SMALL)
    with pytest.raises(ValueError):
        FV.far(torch.zeros(3, 4, 5), SMALL[0], device="cpu", thresholds=SMALL)
    with pytest.raises(ValueError):
        FV.far(torch.zeros(3, 8), SMALL[0], device="cpu", ld=4)
