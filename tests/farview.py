"""Far views for kernel tests: a small logical operand whose row stride is so large that its last row lies more than 2^31
bytes, 2^32 bytes or 2^31 elements from its base (the red zones of tests/redzone.py at far offsets).

    v = far(a_cpu, B32, POISON)           # values of the 2-D a_cpu, ld chosen so that the last row starts just past 2^32 bytes
    kernel(v, v.stride(0), ...)
    check_untouched(v)                    # every byte of the parent outside the logical elements still holds the fill

Only rows x cols elements are ever written or compared; the parent is one allocation of about `reach` bytes holding the fill.
Every view crosses each threshold at or below its reach (2^31 and 2^32 bytes, 2^33 bytes = 2^31 elements) with at least one
row on either side of it, and no two row offsets are congruent modulo 2^32 bytes: an offset that wrapped in 32 bits lands in
another row's data or in the fill, never on the same values.  Works on CPU tensors with small reaches too
(tests/test_farview_helper.py)."""
import bisect

import torch

import redzone as RZ

B31 = 1 << 31        # farthest byte offset just above 2^31: signed 32-bit byte offsets
B32 = 1 << 32        # just above 2^32: unsigned 32-bit byte offsets, int element index x 4 in 32 bits
E31 = 1 << 33        # just above 2^33 bytes = 2^31 elements: signed 32-bit element indices
REACHES = {"B31": B31, "B32": B32, "E31": E31}
CHUNK = 256 << 20    # check_untouched looks at the parent in slices of at most this many bytes


class _Far:
    """Where the logical rows of a far view lie: parent (uint8), byte offset of the base, element offset of every row from the
    base (ascending), columns, the regular row stride (None for far_rows) and the fill."""

    def __init__(self, parent, off, row_off, cols, ld, isz, fill):
        self.parent, self.off, self.row_off, self.cols, self.ld, self.isz, self.fill = parent, off, list(row_off), cols, ld, isz, fill
        self.rows = len(self.row_off)
        self.starts = [off + r * isz for r in self.row_off]          # first byte of every logical row inside the parent
        assert all(b - a >= cols * isz for a, b in zip(self.starts, self.starts[1:])), "logical rows overlap or are not ascending"

    @property
    def span(self):
        return (self.row_off[-1] + self.cols) * self.isz


def ld_for(rows, reach, isz=4, thresholds=(B31, B32, E31)):
    """The row stride (elements, a multiple of 4) that puts the last of `rows` rows just past `reach` bytes, with at least one
    row on each side of every threshold <= reach and distinct row offsets modulo 2^32 bytes."""
    if rows < 2:
        raise ValueError("a far view needs at least two rows")
    ld = -(-(reach + isz) // ((rows - 1) * isz))
    ld += -ld % 4
    while True:
        offs = [r * ld * isz for r in range(rows)]
        ok = offs[-1] > reach and len({o % (1 << 32) for o in offs}) == rows
        for th in thresholds:
            if th <= reach:
                ok = ok and any(o < th for o in offs) and any(o >= th for o in offs)
        if ok:
            return ld
        ld += 4


def far(t, reach, fill=RZ.POISON, device="cuda", ld=None, thresholds=(B31, B32, E31)):
    """A view on `device` with the values of the small 2-D CPU tensor `t`, unit inner stride and a row stride that puts its last
    row just past `reach` bytes from its first element, inside ONE parent allocation whose every other byte is `fill`.  The base
    is 256-byte aligned.  `ld` overrides the computed stride (boundary cases)."""
    if t.dim() != 2 or t.dtype not in RZ.DTYPES:
        raise ValueError("far: a 2-D tensor of one of %s" % (RZ.DTYPES,))
    rows, cols = t.shape
    isz = t.element_size()
    if ld is None:
        ld = ld_for(rows, reach, isz, thresholds)
    if ld < cols:
        raise ValueError("far: ld %d for %d columns" % (ld, cols))
    span = ((rows - 1) * ld + cols) * isz
    total = RZ.MARGIN + RZ.ALIGN + span + RZ.MARGIN
    total += -total % 8
    parent = torch.empty(total, dtype=torch.uint8, device=device)
    parent.fill_(fill)
    off = RZ.MARGIN + (-(parent.data_ptr() + RZ.MARGIN)) % RZ.ALIGN
    view = torch.as_strided(parent[off: off + span].view(t.dtype), (rows, cols), (ld, 1))
    view.copy_(t.to(device))
    assert view.data_ptr() == parent.data_ptr() + off and view.data_ptr() % RZ.ALIGN == 0
    view._far = _Far(parent, off, [r * ld for r in range(rows)], cols, ld, isz, fill)
    return view


def far_rows(t, at, ld, fill=RZ.POISON, device="cuda"):
    """Sparse logical rows of a huge row-major matrix: row i of the 2-D CPU tensor `t` lies at row index at[i] (ascending) of a
    matrix with row stride `ld`, inside ONE parent of (max(at) * ld + columns) elements holding `fill`.  Returns the whole matrix
    as a view [max(at) + 1, columns] with strides (ld, 1): index it with `at` to read the logical rows back.  What the engine's
    position-major buffers look like to a kernel that is handed a few sequences of a very large micro-batch."""
    if t.dim() != 2 or t.dtype not in RZ.DTYPES or len(at) != t.shape[0] or ld < t.shape[1]:
        raise ValueError("far_rows: a 2-D tensor of one of %s, one row index per row, ld >= columns" % (RZ.DTYPES,))
    at = [int(a) for a in at]
    cols, isz = t.shape[1], t.element_size()
    span = (at[-1] * ld + cols) * isz
    total = RZ.MARGIN + RZ.ALIGN + span + RZ.MARGIN
    total += -total % 8
    parent = torch.empty(total, dtype=torch.uint8, device=device)
    parent.fill_(fill)
    off = RZ.MARGIN + (-(parent.data_ptr() + RZ.MARGIN)) % RZ.ALIGN
    view = torch.as_strided(parent[off: off + span].view(t.dtype), (at[-1] + 1, cols), (ld, 1))
    view._far = _Far(parent, off, [a * ld for a in at], cols, None, isz, fill)
    view[torch.tensor(at, device=device)] = t.to(device)
    assert view.data_ptr() == parent.data_ptr() + off and view.data_ptr() % RZ.ALIGN == 0
    return view


def farthest(view):
    """Byte offset of the last logical row from the view's base."""
    f = view._far
    return f.row_off[-1] * f.isz


def damage(view, chunk=CHUNK):
    """None, or a description of the first 8-byte word outside the logical elements that no longer holds the fill.  The parent
    is compared in slices of at most `chunk` bytes viewed as int64 (one bool per word: chunk / 8 bytes of extra memory plus the
    comparison's operand); the logical rows inside a slice are saved, overwritten with the fill for the comparison and put
    back."""
    f = view._far
    p = f.parent
    n = p.numel()
    assert n % 8 == 0 and chunk % 8 == 0
    word = int(torch.full((8,), f.fill, dtype=torch.uint8).view(torch.int64))
    width = f.cols * f.isz
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        saved = []
        i = bisect.bisect_left(f.starts, lo - width + 1)            # the logical rows whose bytes intersect [lo, hi)
        while i < f.rows and f.starts[i] < hi:
            a, b = max(f.starts[i], lo), min(f.starts[i] + width, hi)
            if a < b:
                saved.append((a, b, p[a:b].clone()))
                p[a:b] = f.fill
            i += 1
        bad = p[lo:hi].view(torch.int64) != word
        hit = bool(bad.any())
        if hit:
            at = lo + 8 * int(torch.nonzero(bad)[0])
            at += int(torch.nonzero(p[at: at + 8].cpu() != f.fill)[0])
            value = int(p[at])
        for a, b, keep in saved:
            p[a:b] = keep
        if hit:
            rel = at - f.off
            if rel < 0:
                where = "%d bytes in front of the view" % -rel
            elif rel >= f.span:
                where = "%d bytes behind the view" % (rel - f.span)
            elif f.ld:
                step = f.ld * f.isz
                where = "in the ld gap: row %d, column %d (ld %d, %d columns)" % (rel // step, (rel % step) // f.isz, f.ld, f.cols)
            else:
                below = bisect.bisect_right(f.starts, at) - 1
                where = "between the logical rows: %d bytes past the start of logical row %d" % (at - f.starts[below], below)
            return "byte 0x%02x (fill 0x%02x) at parent byte %d, view byte %d (mod 2^32: %d; mod 2^31: %d): %s" % (
                value, f.fill, at, rel, rel % (1 << 32), rel % (1 << 31), where)
    return None


def check_untouched(view, what="", chunk=CHUNK):
    """Assert that every byte of the view's parent outside its logical elements still holds the fill."""
    if view.is_cuda:
        torch.cuda.synchronize()
    found = damage(view, chunk)
    assert found is None, "%s: %s" % (what or "far view", found)
