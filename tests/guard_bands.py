"""Guard bands: hold a kernel to the memory it was given.

A comparison with a reference sees what a kernel writes where it should write.  These helpers see where ELSE it writes and
whether its result depends on memory that was never part of the call:

  banded(shape, dtype, fill=...)  an output view inside a larger buffer: `rows` guard rows in front and behind, `cols`
                                  guard columns left and right, all holding `fill`; check() compares every guard element
                                  with the fill pattern AS BITS on the tensor's device (one host read) and names the first
                                  damaged (row, column) of the whole buffer.
  exact_workspace(nbytes)         a byte view of exactly nbytes, 256-byte aligned, inside a buffer of 0xA5 bytes whose
                                  bands in front and behind are at least max(64 KiB, nbytes // 4) long: wider than the 25 %
                                  slack ops.workspace() has always granted, so whatever worked before lands in the band.
  poisoned_input(t)               t copied into a larger buffer whose guard rows and columns are NaN (floating-point payload
                                  operands ONLY; index operands get guard_index()).
  banded_vector(n, dtype, ...)    the same for a 1-D vector (gamma, mean, db, statistics, the optimizer's flat tensors): `guard`
  poisoned_vector(t)              elements in front and behind, the alignment class (data_ptr() % 16) chosen by the caller.
  guard_index(idx, none=...)      an index array whose guard entries stay valid for the call: -1 where the ABI defines it as
                                  "none", otherwise a copy of the last real entry.  An over-read never becomes a wild access.

Plain module (imported by the tests that use it): no fixtures, no pytest settings.
"""
import torch

_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """The same memory as integers of the element size (NaN == NaN, -0.0 != 0.0)."""
    return t.view(_INT_OF[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def _aligned_base(numel, dtype, device, align):
    """A 1-D tensor of `numel` elements whose data_ptr() % 16 == align % 16 (align in bytes: 0 or 8)."""
    es = torch.empty(0, dtype=dtype).element_size()
    assert align in (0, 8) and 16 % es == 0 and align % es == 0
    raw = torch.empty(numel + 32 // es, dtype=dtype, device=device)
    off = ((align - raw.data_ptr()) % 16) // es
    return raw[off:off + numel]


class Band:
    """The buffer around one inner view.  Guard regions, in coordinates of the whole buffer (R rows x ld columns):
    'front' rows [0, rows), 'behind' rows [rows + n, R), 'left' columns [0, c0) and 'right' columns [c0 + c, ld) of the
    inner rows.  `c0` counts the alignment shift of the inner view's first column."""

    def __init__(self, buf, r0, n, c0, c, fill_bits, name):
        self.buf, self.r0, self.n, self.c0, self.c, self.name = buf, r0, n, c0, c, name
        self.fill_bits = fill_bits

    def region(self, which):
        b, r0, n, c0, c = self.buf, self.r0, self.n, self.c0, self.c
        return {"front": b[:r0], "behind": b[r0 + n:], "left": b[r0:r0 + n, :c0], "right": b[r0:r0 + n, c0 + c:]}[which]

    def damaged(self):
        """None, or (row, column, which) of the first damaged guard element in row-major order of the whole buffer."""
        bad = bits(self.buf) != self.fill_bits
        bad[self.r0:self.r0 + self.n, self.c0:self.c0 + self.c] = False
        flat = bad.reshape(-1)
        cnt = flat.sum()
        first = torch.argmax(flat.to(torch.uint8))
        cnt, first = torch.stack([cnt, first]).tolist()  # the one host read
        if cnt == 0:
            return None
        ld = self.buf.shape[1]
        r, col = first // ld, first % ld
        which = "front" if r < self.r0 else "behind" if r >= self.r0 + self.n else "left" if col < self.c0 else "right"
        return r, col, which, cnt

    def check(self):
        d = self.damaged()
        assert d is None, (f"{self.name}: guard band damaged: {d[3]} element(s), the first at buffer (row {d[0]}, column {d[1]}) "
                           f"= inner (row {d[0] - self.r0}, column {d[1] - self.c0}), in the '{d[2]}' guard")


def _fill_bits(fill, dtype):
    return int(bits(torch.tensor([fill], dtype=dtype)).item())


def banded(shape, dtype, *, rows=256, cols=8, fill, align=0, ld=None, device="cuda", name="out"):
    """-> (inner view of `shape` (n, c), Band).  Every element, inner ones included, starts as `fill`.
    align: data_ptr() % 16 of the inner view (0, or 8 = 8-byte but not 16-byte aligned; 4-byte elements also 4 or 12);
    ld: row stride in elements (default c + 2 * cols rounded up so that every row keeps the alignment class)."""
    n, c = shape
    es = torch.empty(0, dtype=dtype).element_size()
    per16 = 16 // es
    # left guard: `cols` rounded up to whole 16-byte groups (the base of the buffer is 16-byte aligned), plus the alignment shift
    c0 = -(-cols // per16) * per16 + align // es
    if ld is None:  # (no guard columns and no shift: contiguous rows, for entry points that know no row stride)
        ld = c if (cols == 0 and align == 0) else -(-(c0 + c + cols) // per16) * per16
    assert ld >= c0 + c + cols, f"ld = {ld} leaves no room for {cols} guard columns on both sides of {c} columns"
    flat = _aligned_base((n + 2 * rows) * ld, dtype, device, 0)
    bits(flat).fill_(_fill_bits(fill, dtype))
    buf = flat.view(n + 2 * rows, ld)
    inner = buf[rows:rows + n, c0:c0 + c]
    # (row 0 of the inner view: with a row stride that is no multiple of 16 bytes the later rows alternate)
    assert (rows * ld * es) % 16 == 0 and inner.data_ptr() % 16 == align
    return inner, Band(buf, rows, n, c0, c, _fill_bits(fill, dtype), name)


def poisoned_input(t, rows=256, *, cols=8, align=0, ld=None, name="in"):
    """-> (inner view holding t's values, Band whose guards are NaN).  Floating-point payload operands only."""
    assert t.is_floating_point() and t.dim() == 2
    inner, band = banded(tuple(t.shape), t.dtype, rows=rows, cols=cols, fill=float("nan"), align=align, ld=ld, device=t.device,
                         name=name)
    inner.copy_(t)
    return inner, band


def banded_vector(n, dtype, *, fill, guard=256, align=0, device="cuda", name="vec"):
    """-> (1-D inner view of n elements, Band): `guard` elements (at least; whole 16-byte groups) holding `fill` in front and
    behind, the inner view included.  align: data_ptr() % 16 of the inner view, any multiple of the element size below 16
    (fp32: 0, 4, 8 or 12 - the alignment class the caller's entry point is to be shown).  The Band is that of a one-row
    buffer: a damaged element is reported in its 'left' (in front) or 'right' (behind) guard with inner column = its index."""
    es = torch.empty(0, dtype=dtype).element_size()
    assert 0 <= align < 16 and align % es == 0, f"align = {align} is no alignment class of {es}-byte elements"
    per16 = 16 // es
    c0 = -(-guard // per16) * per16 + align // es
    total = c0 + n + guard + per16
    flat = _aligned_base(total, dtype, device, 0)
    bits(flat).fill_(_fill_bits(fill, dtype))
    buf = flat.view(1, total)
    inner = buf[0, c0:c0 + n]
    assert inner.data_ptr() % 16 == align and total - c0 - n >= guard
    return inner, Band(buf, 0, 1, c0, n, _fill_bits(fill, dtype), name)


def poisoned_vector(t, *, guard=256, align=0, name="vec"):
    """-> (1-D inner view holding t's values, Band whose guard elements are NaN).  Floating-point vectors only."""
    assert t.is_floating_point() and t.dim() == 1
    inner, band = banded_vector(t.numel(), t.dtype, fill=float("nan"), guard=guard, align=align, device=t.device, name=name)
    inner.copy_(t)
    return inner, band


def guard_index(idx, *, none=None, rows=256):
    """A copy of the 1-D or 2-D index tensor with `rows` guard entries (rows) in front and behind that are VALID for the call:
    `none` (-1) where the ABI defines it, otherwise the first / last real entry.  -> (inner view, check) where check() asserts
    that the guards still hold those values (index operands are inputs: nothing may write them)."""
    n = idx.shape[0]
    buf = torch.empty((n + 2 * rows,) + tuple(idx.shape[1:]), dtype=idx.dtype, device=idx.device)
    if none is not None or n == 0:
        buf.fill_(-1 if none is None else none)
    else:
        buf[:rows] = idx[:1]
        buf[rows + n:] = idx[-1:]
    buf[rows:rows + n] = idx
    want = buf.clone()

    def check():
        assert torch.equal(buf, want), "an index operand (or its guard entries) was written"

    return buf[rows:rows + n], check


class WorkspaceBand:
    FILL = 0xA5

    def __init__(self, buf, start, nbytes):
        self.buf, self.start, self.nbytes = buf, start, nbytes

    def damaged(self):
        bad = self.buf != self.FILL
        bad[self.start:self.start + self.nbytes] = False
        cnt, first = torch.stack([bad.sum(), torch.argmax(bad.to(torch.uint8))]).tolist()
        if cnt == 0:
            return None
        return ("front", first - self.start, cnt) if first < self.start else ("behind", first - self.start - self.nbytes, cnt)

    def check(self):
        d = self.damaged()
        assert d is None, (f"workspace of exactly {self.nbytes} bytes: {d[2]} byte(s) written outside it, the first "
                           + (f"{-d[1]} byte(s) in front of it" if d[0] == "front" else f"at byte {d[1]} behind its end"))


def exact_workspace(nbytes, device="cuda"):
    """-> (uint8 view of exactly nbytes, 256-byte aligned; WorkspaceBand).  The whole buffer, the view included, holds 0xA5."""
    nbytes = int(nbytes)
    band = max(64 << 10, nbytes // 4)
    raw = torch.full((2 * band + nbytes + 512,), WorkspaceBand.FILL, dtype=torch.uint8, device=device)
    start = band + (-(raw.data_ptr() + band)) % 256
    view = raw[start:start + nbytes]
    assert view.data_ptr() % 256 == 0 and view.numel() == nbytes and raw.numel() - start - nbytes >= band
    return view, WorkspaceBand(raw, start, nbytes)


class ExactWorkspaces:
    """Stands in for ops.workspace: every request is served by a fresh exact-size view; check() verifies every band handed
    out so far.  `monkeypatch.setattr(ops, "workspace", ExactWorkspaces())`."""

    def __init__(self):
        self.served = []

    def __call__(self, nbytes, device):
        view, band = exact_workspace(nbytes, device)
        self.served.append(band)
        return view

    def check(self, at_least=1):
        assert len(self.served) >= at_least, f"expected at least {at_least} workspace request(s), saw {len(self.served)}"
        for b in self.served:
            b.check()
