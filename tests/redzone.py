"""Red zones for kernel tests: operands and outputs embedded in a larger buffer whose every other byte holds a known fill, so
that a read outside a tensor changes the result and a write outside it is found byte for byte.

    g = Guard(POISON)
    a = g.embed(a_cpu, ld=K + 8)          # values of a_cpu, row stride K + 8, fill in the ld gap, in front and behind
    out = g.embed(torch.zeros(M, N), ld=N + 8)
    kernel(a, ..., out)
    g.check()                             # every byte outside the views still holds the fill

Two fills: ZERO (all bytes 0x00) and POISON (all bytes 0xFF: a quiet NaN as fp32 / fp16 / bf16, -1 as int32 / int64, 255 as
uint8).  A kernel whose result depends on memory it was not given differs between the two (assert_same_bits).  Imported by
the tests like beam_ref.py; works on CPU tensors too (tests/test_redzone_helper.py)."""
import torch

ZERO = 0x00
POISON = 0xFF
MARGIN = 4096        # bytes of fill in front of and behind every view (at least)
ALIGN = 256          # every view starts at a multiple of this address
DTYPES = (torch.float32, torch.int32, torch.int64, torch.uint8)
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class _View:
    def __init__(self, name, parent, off, rows, cols, ld, isz):
        self.name, self.parent, self.off, self.rows, self.cols, self.ld, self.isz = name, parent, off, rows, cols, ld, isz

    @property
    def span(self):
        return ((self.rows - 1) * self.ld + self.cols) * self.isz if self.rows and self.cols else 0

    def damage(self, fill):
        """None, or a description of the first byte outside the view that no longer holds `fill`."""
        p = self.parent
        outside = torch.ones(p.numel(), dtype=torch.bool, device=p.device)
        if self.span:
            if self.ld == self.cols:
                outside[self.off: self.off + self.span] = False
            else:
                r = torch.arange(self.rows, device=p.device)[:, None] * (self.ld * self.isz)
                c = torch.arange(self.cols * self.isz, device=p.device)[None, :]
                outside[(self.off + r + c).reshape(-1)] = False
        bad = outside & (p != fill)
        if not bool(bad.any()):
            return None
        at = int(torch.nonzero(bad)[0])
        value = int(p[at])
        if at < self.off:
            where = "%d bytes (%d elements) in front of the view" % (self.off - at, -(-(self.off - at) // self.isz))
        elif at >= self.off + self.span:
            d = at - (self.off + self.span)
            where = "%d bytes (element %d) behind the view" % (d, d // self.isz)
        else:
            rel = at - self.off
            where = "in the ld gap: row %d, column %d (ld %d, %d columns)" % (
                rel // (self.ld * self.isz), (rel % (self.ld * self.isz)) // self.isz, self.ld, self.cols)
        return "%s: byte 0x%02x (fill 0x%02x) %s" % (self.name, value, fill, where)


def embed(t, ld=None, fill=POISON, guard=None, device="cuda", name=None):
    """A tensor on `device` with the values and shape of `t`, unit inner stride and row stride `ld` (default: tight), inside a
    parent buffer whose every other byte is `fill`.  ld > columns needs a 2-D `t`.  `guard` remembers the parent."""
    if t.dtype not in DTYPES:
        raise TypeError("embed: %s is not one of %s" % (t.dtype, DTYPES))
    shape = tuple(t.shape)
    cols = shape[-1] if shape else 1
    rows = 1
    for s in shape[:-1]:
        rows *= s
    if ld is None or t.dim() < 2:
        ld = cols
    if ld < cols or (ld > cols and t.dim() != 2):
        raise ValueError("embed: ld=%d for a tensor of shape %s" % (ld, shape))
    isz = t.element_size()
    v = _View(name or "view %d" % (len(guard.views) if guard is not None else 0), None, 0, rows, cols, ld, isz)
    span = v.span
    parent = torch.full((MARGIN + ALIGN + span + MARGIN,), fill, dtype=torch.uint8, device=device)
    v.parent = parent
    v.off = MARGIN + (-(parent.data_ptr() + MARGIN)) % ALIGN
    flat = parent[v.off: v.off + span].view(t.dtype)
    if ld == cols:
        out = flat.reshape(shape)
    else:
        out = torch.as_strided(flat, (rows, cols), (ld, 1))
    out.copy_(t)
    assert not span or (out.data_ptr() == parent.data_ptr() + v.off and out.data_ptr() % ALIGN == 0)
    if guard is not None:
        guard.views.append(v)
    return out


class Guard:
    """Remembers the parents of its embeds; check() asserts that every byte outside the views still holds the fill."""

    def __init__(self, fill=POISON, device="cuda"):
        self.fill, self.device, self.views = fill, device, []

    def embed(self, t, ld=None, name=None):
        return embed(t, ld=ld, fill=self.fill, guard=self, device=self.device, name=name)

    def opt(self, t, ld=None, name=None):
        """embed(), or None for None (optional operands)."""
        return None if t is None else self.embed(t, ld=ld, name=name)

    def bytes(self, nbytes, name=None):
        """A guarded uint8 buffer of exactly `nbytes` bytes, itself holding the fill (outputs a kernel writes in its own layout)."""
        return self.embed(torch.full((int(nbytes),), self.fill, dtype=torch.uint8), name=name)

    def check(self):
        if self.device != "cpu":
            torch.cuda.synchronize()
        for v in self.views:
            what = v.damage(self.fill)
            assert what is None, what


def assert_same_bits(a, b, what=""):
    """Equal shape, dtype and bits (through an integer view: equal NaNs compare equal)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    it = _INT_OF_SIZE[a.element_size()]
    ia, ib = a.contiguous().view(it), b.contiguous().view(it).to(a.device)
    if torch.equal(ia, ib):
        return
    diff = torch.nonzero(ia != ib)
    first = tuple(int(i) for i in diff[0])
    raise AssertionError("%s: %d of %d elements differ in their bits, first at %s: %r vs %r" % (
        what, diff.shape[0], ia.numel(), first, a[first].item(), b[first].item()))
