"""CPU: tests/redzone.py is not vacuous -- a store one element outside a view, or into an ld gap, is reported with its place; a
torch op evaluated over one row or column too many of a POISON embed yields NaN; alignment, margins and contiguity hold for
every supported dtype."""
import pytest
import torch

import redzone as RZ


def _values(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return torch.randn(*shape, generator=g)
    return torch.randint(0, 100, shape, generator=g).to(dtype)


def _beyond(view, elements):
    """A 1-D view of `elements` elements starting at view's first element (reaches past its end, or in front of it when the
    storage offset allows: the helper's own parent is the storage)."""
    return torch.as_strided(view, (elements,), (1,))


@pytest.mark.parametrize("dtype", RZ.DTYPES)
@pytest.mark.parametrize("fill", [RZ.ZERO, RZ.POISON])
def test_embed_keeps_values_alignment_margins_and_contiguity(dtype, fill):
    for shape, ld in (((5, 7), None), ((5, 7), 15), ((1, 7), 15), ((3, 4, 6), None), ((9,), None), ((2, 0), None), ((1, 1), 9)):
        g = RZ.Guard(fill, device="cpu")
        t = _values(shape, dtype)
        v = g.embed(t, ld=ld)
        rec = g.views[-1]
        assert v.dtype == dtype and tuple(v.shape) == shape and torch.equal(v, t)
        if v.numel():                        # (torch gives an empty tensor no address)
            assert v.data_ptr() % RZ.ALIGN == 0 and v.stride(-1) == 1
            assert v.data_ptr() - rec.parent.data_ptr() >= RZ.MARGIN                                     # fill in front
            assert rec.parent.data_ptr() + rec.parent.numel() - (v.data_ptr() + rec.span) >= RZ.MARGIN   # and behind
        if ld is None:
            assert v.is_contiguous()
        elif shape[0] > 1:
            assert v.stride(0) == ld and not v.is_contiguous()
        # every byte of the parent outside the view is the fill
        assert int((rec.parent != fill).sum()) <= v.numel() * v.element_size()
        g.check()


def test_the_two_fills_read_as_documented():
    nan = RZ.embed(torch.zeros(2, 3), ld=5, fill=RZ.POISON, device="cpu")
    gap = torch.as_strided(nan, (2, 5), (5, 1))[0, 3:]
    assert torch.isnan(gap).all()
    for dt in (torch.float16, torch.bfloat16):
        assert torch.isnan(torch.full((4,), RZ.POISON, dtype=torch.uint8).view(dt)).all()
    assert int(torch.full((4,), RZ.POISON, dtype=torch.uint8).view(torch.int32)) == -1
    assert int(torch.full((8,), RZ.POISON, dtype=torch.uint8).view(torch.int64)) == -1
    zero = RZ.embed(torch.ones(2, 3), ld=5, fill=RZ.ZERO, device="cpu")
    assert (torch.as_strided(zero, (2, 5), (5, 1))[0, 3:] == 0).all()


@pytest.mark.parametrize("dtype", RZ.DTYPES)
@pytest.mark.parametrize("fill", [RZ.ZERO, RZ.POISON])
def test_a_store_one_element_behind_a_view_is_reported(dtype, fill):
    g = RZ.Guard(fill, device="cpu")
    v = g.embed(_values((4, 6), dtype), name="out")
    g.check()
    _beyond(v, 25)[24] = 7                                   # element 24 is the first one behind the 4 x 6 view
    with pytest.raises(AssertionError, match=r"out: .*\(element 0\) behind the view"):
        g.check()


@pytest.mark.parametrize("dtype", RZ.DTYPES)
def test_a_store_one_element_in_front_of_a_view_is_reported(dtype):
    g = RZ.Guard(RZ.POISON, device="cpu")
    v = g.embed(_values((4, 6), dtype), ld=9, name="out")
    rec = g.views[-1]
    isz = v.element_size()
    front = rec.parent[rec.off - isz: rec.off].view(dtype)   # the element in front of the view
    front[0] = 7
    with pytest.raises(AssertionError, match=r"out: .*\(1 elements\) in front of the view"):
        g.check()


@pytest.mark.parametrize("dtype", RZ.DTYPES)
@pytest.mark.parametrize("fill", [RZ.ZERO, RZ.POISON])
def test_a_store_into_an_ld_gap_is_reported_with_row_and_column(dtype, fill):
    g = RZ.Guard(fill, device="cpu")
    v = g.embed(_values((4, 6), dtype), ld=9, name="c")
    other = g.embed(_values((3, 3), dtype), ld=4, name="other")
    g.check()
    torch.as_strided(v, (4, 9), (9, 1))[2, 6] = 7           # row 2, the first column past the 6 the view has
    with pytest.raises(AssertionError, match=r"c: .* in the ld gap: row 2, column 6 "):
        g.check()
    torch.as_strided(v, (4, 9), (9, 1))[2, 6:7].view(torch.uint8).fill_(fill)     # mended: clean again
    g.check()
    v[3, 5] = 9                                              # stores inside a view are not damage
    other[2, 2] = 9
    g.check()


def test_an_op_over_one_row_or_column_too_many_of_a_poison_embed_is_nan():
    """What the GPU tests rely on: a reduction that reads past an operand's edge sees NaN under POISON and the clean value
    under ZERO, so the two runs differ in their bits."""
    a, w = _values((5, 8), torch.float32, 1), _values((3, 8), torch.float32, 2)
    outs = {}
    for fill in (RZ.ZERO, RZ.POISON):
        g = RZ.Guard(fill, device="cpu")
        ea, ew = g.embed(a, ld=12), g.embed(w)
        good = ea @ ew.t()
        assert torch.isfinite(good).all() and torch.equal(good, a @ w.t())
        wide_a = torch.as_strided(ea, (5, 9), (12, 1))                        # one column too many (K tail not masked)
        wide_w = torch.cat([ew, torch.ones(3, 1)], dim=1)
        tall_w = torch.as_strided(ew, (4, 8), (8, 1))                         # one row too many (N edge not masked)
        outs[fill] = (wide_a @ wide_w.t(), (ea @ tall_w.t())[:, :3], torch.softmax(wide_a, dim=1)[:, :8])
        g.check()                                                              # (reads damage nothing)
    assert torch.equal(outs[RZ.ZERO][0], a @ w.t())                            # the ZERO run hides the column
    assert torch.isnan(outs[RZ.POISON][0]).all()                               # the POISON run shows it
    assert torch.isnan(outs[RZ.POISON][2]).all() and torch.isfinite(outs[RZ.ZERO][2]).all()
    RZ.assert_same_bits(outs[RZ.ZERO][1], outs[RZ.POISON][1])                  # rows past the edge that are then dropped: equal
    with pytest.raises(AssertionError, match="differ in their bits"):
        RZ.assert_same_bits(outs[RZ.ZERO][0], outs[RZ.POISON][0], "k tail")
    # integer operands: a token read one element too far is -1 / 255, not a plausible index
    tok = RZ.embed(torch.tensor([3, 1, 2], dtype=torch.int32), fill=RZ.POISON, device="cpu")
    assert _beyond(tok, 4).tolist() == [3, 1, 2, -1]
    msk = RZ.embed(torch.tensor([0, 1], dtype=torch.uint8), fill=RZ.POISON, device="cpu")
    assert _beyond(msk, 3).tolist() == [0, 1, 255]


def test_assert_same_bits_treats_equal_nans_as_equal_and_signed_zeros_as_different():
    a = torch.tensor([1.0, float("nan"), 0.0])
    RZ.assert_same_bits(a, a.clone())
    with pytest.raises(AssertionError):
        RZ.assert_same_bits(a, torch.tensor([1.0, float("nan"), -0.0]))
    with pytest.raises(AssertionError):
        RZ.assert_same_bits(a, a.double())
    with pytest.raises(AssertionError):
        RZ.assert_same_bits(a, a[:2])
    RZ.assert_same_bits(torch.arange(6).view(2, 3), torch.arange(6).view(2, 3))


def test_guard_bytes_is_a_guarded_buffer_of_exactly_that_size():
    g = RZ.Guard(RZ.POISON, device="cpu")
    b = g.bytes(1000, name="planes")
    assert b.numel() == 1000 and b.dtype == torch.uint8 and (b == RZ.POISON).all()
    b.zero_()
    g.check()
    _beyond(b, 1001)[1000] = 0
    with pytest.raises(AssertionError, match=r"planes: .*\(element 0\) behind the view"):
        g.check()
