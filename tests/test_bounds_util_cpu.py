"""tests/bounds_util.py on CPU tensors: the guarded view is contiguous, sits at the stated byte offset and has poison on
both sides; a canary handle notices one overwritten word in front or behind; ``extent`` is exact."""
import math

import pytest
import torch

import bounds_util as B

CPU = torch.device("cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.int64])
@pytest.mark.parametrize("poison", B.POISONS)
def test_guarded_view_sits_in_the_middle_of_poison(dtype, poison):
    t = (torch.arange(2 * 3 * 5 * 7).reshape(2, 3, 5, 7) % 97).to(dtype)
    v = B.guarded(CPU, t, poison)
    assert v.is_contiguous() and v.shape == t.shape and v.dtype == dtype and torch.equal(v, t)
    assert v.data_ptr() % 256 == v.untyped_storage().data_ptr() % 256          # the allocation's alignment is kept
    assert v.data_ptr() - v.untyped_storage().data_ptr() == B.PAD_BYTES
    assert v.untyped_storage().nbytes() == 2 * B.PAD_BYTES + t.numel() * t.element_size()
    lead = B.PAD_BYTES // t.element_size()
    flat = torch.empty(0, dtype=dtype).set_(v.untyped_storage())
    for side in (flat[:lead], flat[lead + t.numel():]):
        assert side.numel() == lead
        if not dtype.is_floating_point:
            assert bool((side.abs() >= 1 << 30).all())                         # far outside any statistic of the tests
        elif math.isnan(poison):
            assert bool(torch.isnan(side).all())
        else:
            assert bool((side.float().abs() == poison).all())                  # exactly representable in every format
            assert bool((side.float() > 0).any()) and bool((side.float() < 0).any())
    v.zero_()                                                                  # the view aliases the buffer's middle only
    assert bool((flat[lead:lead + t.numel()] == 0).all()) and not bool((flat[:lead] == 0).any())


@pytest.mark.parametrize("dtype,fill", [(torch.float32, float("nan")), (torch.bfloat16, 0.0), (torch.int64, 0)])
def test_canary_handle_notices_one_word(dtype, fill):
    h = B.with_canary(CPU, (3, 5), dtype, fill, extra_bytes=256)
    item = h.flat.element_size()
    assert h.view.is_contiguous() and tuple(h.view.shape) == (3, 5) and h.count == 15 and h.lead == B.PAD_BYTES // item
    assert h.view.data_ptr() - h.flat.data_ptr() == B.PAD_BYTES
    assert h.flat.numel() == h.lead + 15 + 256 // item
    if isinstance(fill, float) and math.isnan(fill):
        assert bool(torch.isnan(h.view).all())
    else:
        assert bool((h.view == fill).all())
    assert B.intact(h)
    h.view.fill_(1)                                   # writing the whole view is what a kernel is allowed to do
    assert B.intact(h)
    assert not B.intact(h, end=14)                    # ... and is an overrun of a view that ends one element earlier
    for pos in (h.lead + 15, h.flat.numel() - 1, 0, h.lead - 1):
        saved = h.flat[pos].clone()
        h.flat[pos] = 1
        assert not B.intact(h), pos
        h.flat[pos] = saved
        assert B.intact(h)
    with pytest.raises(ValueError):
        B.with_canary(CPU, (4,), dtype, fill, extra_bytes=0)


def test_canary_behind_a_short_view_of_a_workspace():
    """The workspace layout of the weight-gradient tests: a leading view, everything behind it canary."""
    h = B.with_canary(CPU, (10,), torch.float32, B.CANARY_F, extra_bytes=4 * 30)
    assert h.flat.numel() == h.lead + 40 and B.intact(h)
    ws = h.flat[h.lead:]
    assert B.extent(ws, B.CANARY_F) == 0
    ws[:10] = 2.0
    assert B.intact(h) and B.extent(ws, B.CANARY_F) == 10
    ws[17] = 0.0
    assert not B.intact(h) and B.extent(ws, B.CANARY_F) == 18


def test_extent_is_exact():
    ws = torch.full((1000,), B.CANARY_F)
    assert B.extent(ws, B.CANARY_F) == 0
    ws[0] = 1.0
    assert B.extent(ws, B.CANARY_F) == 1
    ws[617] = float("nan")                            # a NaN differs from a finite sentinel
    assert B.extent(ws, B.CANARY_F) == 618
    ws[999] = 0.0
    assert B.extent(ws, B.CANARY_F) == 1000
    nan = torch.full((64,), float("nan"))
    assert B.extent(nan, float("nan")) == 0
    nan[40] = B.CANARY_F
    assert B.extent(nan, float("nan")) == 41
    assert B.extent(nan.view(8, 8), float("nan")) == 41
    ints = torch.full((33,), B.CANARY_I, dtype=torch.int64)
    ints[32] = 0
    assert B.extent(ints, B.CANARY_I) == 33
