"""Buffers with a fence on either side: a launch that stores in front of or behind what it was given, or that reads scratch it never wrote, shows.

A Fence owns band + nbytes + band bytes.  The bands hold a sentinel byte and must still hold it afterwards; the interior -- what the kernel is handed --
starts out as poison: all-ones bytes, a NaN as fp16, fp32 and fp64 and 255 as a byte, so a value read before it was written spoils every comparison
downstream.  Plain tensor code, on the GPU and on the CPU alike (tests/test_fenced_host.py proves on CPU tensors that check() can fail)."""
import contextlib

import torch

ALIGN = 256
_empty = torch.empty           # (FencedAllocations replaces torch.empty while it is active; a Fence's own buffer never comes from there)


class Fence:
    def __init__(self, nbytes, band, device, poison=0xFF, sentinel=0xA5, stream=None):
        """nbytes: the interior, exactly; band: bytes on each side, rounded up to a multiple of 256, so the interior stays 256-B aligned; stream: allocate and
        fill with that stream current (the caching allocator then knows it as the owner)."""
        self.nbytes, self.sentinel, self.poison = int(nbytes), sentinel, poison
        self.band = (int(band) + ALIGN - 1) // ALIGN * ALIGN
        total = 2 * self.band + self.nbytes
        device = torch.device(device)
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            raw = _empty(total + ALIGN - 1, dtype=torch.uint8, device=device)
            first = -raw.data_ptr() % ALIGN
            self.buffer = raw[first:first + total]
            self.buffer.fill_(sentinel)
            self.view = self.buffer[self.band:self.band + self.nbytes]
            self.view.fill_(poison)
        assert self.view.data_ptr() % ALIGN == 0

    def damage(self):
        """(first, last) offsets of the damaged band bytes relative to the interior (negative: in front of it; >= nbytes: behind it), or None"""
        front, back = self.buffer[:self.band], self.buffer[self.band + self.nbytes:]
        bad = torch.cat([torch.nonzero(front != self.sentinel).flatten() - self.band, torch.nonzero(back != self.sentinel).flatten() + self.nbytes])
        if bad.numel() == 0:
            return None
        return int(bad.min()), int(bad.max())

    def check(self, what='buffer'):
        hit = self.damage()
        assert hit is None, '%s of %d bytes: bytes outside it were written, the first at offset %d and the last at offset %d (bands of %d bytes)' % (
            what, self.nbytes, hit[0], hit[1], self.band)

    def untouched(self):
        """the interior still holds nothing but poison"""
        return bool((self.view == self.poison).all())


def fenced_like(shape, dtype, band_elems, device='cuda', channels_last=False, **kw):
    """(tensor, fence): a poisoned tensor of `shape` and `dtype` inside a Fence with band_elems elements on each side.  Contiguous; with channels_last the
    memory is [N][H][W][C] and the tensor its [N, C, H, W] view, what the fp16 kernels take."""
    shape = tuple(int(s) for s in shape)
    size = _empty((), dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= s
    fence = Fence(numel * size, band_elems * size, device, **kw)
    flat = fence.view.view(dtype)
    if channels_last:
        n, c, h, w = shape
        return flat.view(n, h, w, c).permute(0, 3, 1, 2), fence
    return flat.view(shape), fence


class FencedAllocations:
    """While active, every tensor that Python code creates on `device_type` with torch.empty / empty_like / full / full_like / zeros / zeros_like / ones / ones_like /
    randn lies inside a Fence of its own, two images of the tensor (2 x the elements behind its first dimension) wide on each side; empty / empty_like come poisoned.
    So the outputs an op or a test body allocates -- y, dx, dw, images, partial-sum tables, mask bytes -- are fenced at exactly their documented size without the
    body knowing, where the caching allocator would have rounded them up and padded them.  check() after a synchronize."""
    NAMES = ('empty', 'empty_like', 'full', 'full_like', 'zeros', 'zeros_like', 'ones', 'ones_like', 'randn')

    def __init__(self, device_type='cuda'):
        self.device_type = device_type
        self.fences = []                                     # (shape, dtype, still poisoned as handed out, Fence)
        self.orig = {n: getattr(torch, n) for n in self.NAMES}

    # -- the replacements --
    def _mine(self, kw, like=None):
        device = kw.get('device', None if like is None else like.device)
        plain = kw.get('out') is None and not kw.get('pin_memory') and kw.get('layout', torch.strided) is torch.strided and kw.get('names') is None
        return plain and device is not None and torch.device(device).type == self.device_type and (like is None or like.layout is torch.strided)

    def _new(self, shape, kw, dtype, device, channels_last, fill=None):
        shape = tuple(int(v) for v in shape)
        image = 1
        for v in (shape[1:] if len(shape) > 1 else shape):
            image *= v
        t, fence = fenced_like(shape, dtype, 2 * max(image, 1), device=device, channels_last=channels_last and len(shape) == 4)
        self.fences.append((shape, dtype, fill is None, fence))
        if fill is not None:
            t.fill_(fill)
        return t

    @staticmethod
    def _size(args, kw):
        if 'size' in kw:
            return kw['size']
        return args[0] if len(args) == 1 and not isinstance(args[0], int) else args

    def _creator(self, name, fill=None):
        orig = self.orig[name]

        def make(*args, **kw):
            if not self._mine(kw):
                return orig(*args, **kw)
            if name == 'full':
                size, value = (args[0], args[1]) if len(args) > 1 else (self._size(args, kw), kw['fill_value'])
                default = torch.bool if isinstance(value, bool) else torch.int64 if isinstance(value, int) else torch.get_default_dtype()
            else:
                size, value, default = self._size(args, kw), fill, torch.get_default_dtype()
            t = self._new(size, kw, kw.get('dtype') or default, kw['device'], kw.get('memory_format') is torch.channels_last, None if name == 'empty' else value if name != 'randn' else 0)
            if name == 'randn':
                t.normal_(generator=kw.get('generator'))
            return t.requires_grad_() if kw.get('requires_grad') else t
        return make

    def _like(self, name, fill=None):
        orig = self.orig[name]

        def make(like, *args, **kw):
            if not self._mine(kw, like):
                return orig(like, *args, **kw)
            value = (args[0] if args else kw['fill_value']) if name == 'full_like' else fill
            fmt = kw.get('memory_format', torch.preserve_format)
            cl = fmt is torch.channels_last or (fmt is torch.preserve_format and like.dim() == 4 and not like.is_contiguous() and like.is_contiguous(memory_format=torch.channels_last))
            t = self._new(like.shape, kw, kw.get('dtype') or like.dtype, kw.get('device', like.device), cl, value)
            return t.requires_grad_() if kw.get('requires_grad') else t
        return make

    # -- switching --
    def install(self):
        for name, fill in (('empty', None), ('full', None), ('zeros', 0), ('ones', 1), ('randn', None)):
            setattr(torch, name, self._creator(name, fill))
        for name, fill in (('empty_like', None), ('full_like', None), ('zeros_like', 0), ('ones_like', 1)):
            setattr(torch, name, self._like(name, fill))

    def remove(self):
        for name, fn in self.orig.items():
            setattr(torch, name, fn)

    def __enter__(self):
        self.install()
        return self

    def __exit__(self, *exc):
        self.remove()
        return False

    def check(self):
        for i, (shape, dtype, _, fence) in enumerate(self.fences):
            fence.check('tensor %d of %d, %s %s,' % (i, len(self.fences), tuple(shape), dtype))

    def holds(self, t):
        """True when tensor `t` is exactly the interior of one of the fences"""
        return any(f.view.data_ptr() == t.data_ptr() and f.nbytes == t.numel() * t.element_size() for _, _, _, f in self.fences)

    def untouched_since(self, mark):
        """True when every tensor handed out poisoned since fences[mark] still holds nothing but poison"""
        return all(fence.untouched() for _, _, poisoned, fence in self.fences[mark:] if poisoned)
