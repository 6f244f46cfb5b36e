"""The fence of tests/fenced.py on CPU tensors: a byte written just outside the interior or at the far end of a band makes check() fail and name the
offset, a write that fills the interior passes, and an interior nobody wrote reads as NaN in every float format -- the proof that the GPU tests built on it
(tests/test_scratch_bounds_gpu.py) can fail."""
import pytest
import torch

from fenced import Fence, FencedAllocations, fenced_like


@pytest.mark.parametrize('nbytes,band', [(1000, 300), (16, 1), (4096, 65536)])
def test_a_stray_byte_fails_the_check_and_is_named(nbytes, band):
    f = Fence(nbytes, band, 'cpu')
    assert f.band % 256 == 0 and f.band >= band and f.view.numel() == nbytes and f.view.data_ptr() % 256 == 0
    assert f.buffer.numel() == 2 * f.band + nbytes
    f.check()
    for off in (-1, nbytes, -f.band, nbytes + f.band - 1):
        g = Fence(nbytes, band, 'cpu')
        g.buffer[g.band + off] = 0
        assert g.damage() == (off, off)
        with pytest.raises(AssertionError, match=r'first at offset %d and the last at offset %d ' % (off, off)):
            g.check()
    g = Fence(nbytes, band, 'cpu')
    g.buffer[g.band - 3] = 1
    g.buffer[g.band + nbytes + 7] = 1
    assert g.damage() == (-3, nbytes + 7)


def test_a_sentinel_valued_store_into_a_band_is_the_one_blind_spot_and_poison_differs_from_it():
    f = Fence(64, 256, 'cpu')
    assert f.poison != f.sentinel
    f.buffer[0] = f.sentinel
    f.check()


def test_filling_the_interior_passes():
    f = Fence(777, 256, 'cpu')
    assert f.untouched()
    f.view.zero_()
    f.view[-1] = 9
    f.view[0] = 9
    f.check()
    assert not f.untouched()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.float16])
def test_an_untouched_interior_reads_as_nan(dtype):
    f = Fence(512, 256, 'cpu')
    assert bool(torch.isnan(f.view.view(dtype)).all())
    t, g = fenced_like((2, 3, 5, 7), dtype, 2 * 3 * 5 * 7, device='cpu')
    assert t.shape == (2, 3, 5, 7) and t.is_contiguous() and bool(torch.isnan(t).all())
    assert g.band >= 2 * 3 * 5 * 7 * t.element_size()
    t.zero_()
    g.check()
    g.buffer[g.band + g.nbytes] = 0                             # one element past the end of the typed view
    with pytest.raises(AssertionError, match='first at offset %d' % g.nbytes):
        g.check()


def test_channels_last_view():
    t, g = fenced_like((2, 8, 3, 5), torch.float16, 16, device='cpu', channels_last=True)
    assert t.shape == (2, 8, 3, 5) and t.is_contiguous(memory_format=torch.channels_last) and t.stride() == (120, 1, 40, 8)
    assert t.data_ptr() == g.view.data_ptr()
    t.fill_(1.0)
    g.check()
    assert bool((g.view.view(torch.float16) == 1.0).all())


def test_bytes_read_255():
    f = Fence(0, 16, 'cpu')
    assert f.view.numel() == 0
    f.check()
    assert int(Fence(3, 16, 'cpu').view.sum()) == 3 * 255


def test_fenced_allocations_stand_in_for_the_torch_creators():
    """the creation functions ops and test bodies call, through every spelling they use: the tensors behave as before, lie in fences, and a store behind one shows"""
    plain = torch.empty
    with FencedAllocations('cpu') as fa:
        a = torch.empty((2, 3, 4, 5), dtype=torch.float32, device='cpu')
        b = torch.empty(7, dtype=torch.uint8, device=torch.device('cpu'))
        c = torch.empty((2, 8, 3, 5), dtype=torch.float16, device='cpu', memory_format=torch.channels_last)
        d = torch.full((3, 4), float('nan'), device='cpu')
        e = torch.zeros(5, dtype=torch.float64, device='cpu')
        f = torch.ones(2, 2, device='cpu')
        g = torch.empty_like(c)
        h = torch.full_like(a, 2.5)
        i = torch.zeros_like(a.permute(0, 2, 3, 1))
        j = torch.randn(4, 6, device='cpu', generator=torch.Generator().manual_seed(1))
        k = torch.empty(3)                                     # no device named: not ours
        m = torch.ones_like(a, dtype=torch.uint8)
        n = torch.full((2,), 3, device='cpu')
        o = torch.randn(3, 2, device='cpu', requires_grad=True)
    assert torch.empty is plain and len(fa.fences) == 13 and o.requires_grad and o.is_leaf
    assert a.shape == (2, 3, 4, 5) and a.is_contiguous() and bool(torch.isnan(a).all()) and b.shape == (7,) and int(b.sum()) == 7 * 255
    assert c.is_contiguous(memory_format=torch.channels_last) and g.stride() == c.stride() and g.dtype == torch.float16 and bool(torch.isnan(g).all())
    assert bool(torch.isnan(d).all()) and not e.any() and e.dtype == torch.float64 and bool((f == 1).all()) and bool((h == 2.5).all())
    assert i.shape == (2, 4, 5, 3) and not i.any() and j.shape == (4, 6) and bool(torch.isfinite(j).all()) and float(j.std()) > 0.3
    assert k.shape == (3,) and m.dtype == torch.uint8 and int(m.sum()) == a.numel() and n.dtype == torch.int64 and n.tolist() == [3, 3]
    assert fa.untouched_since(0) and fa.holds(a) and fa.holds(c) and not fa.holds(k) and not fa.holds(a[1:])
    fa.check()
    b.fill_(1)
    assert not fa.untouched_since(0)
    fa.check()
    fence = fa.fences[1][3]
    fence.buffer[fence.band + 7] = 0                              # one byte behind the 7-byte tensor, where the allocator's rounding would have hidden it
    with pytest.raises(AssertionError, match='first at offset 7 '):
        fa.check()
