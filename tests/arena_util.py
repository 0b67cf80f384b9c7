"""Guard-banded, deliberately misaligned buffers for the parity tests.

An `Arena` hands out contiguous views laid out as

    [guard: >= 4096 words][pad: `off` words][payload][guard: >= 4096 words]

inside one allocation of their own.  The guard in front starts 256-byte aligned, so `off` (in ELEMENTS of 4 bytes)
alone decides the payload's alignment: off = 1 a 4-byte aligned base, off = 2 an 8-byte aligned one.  Guards, pad words
and the payloads of outputs hold one quiet NaN with a recognisable payload (bits 0x7FC0BEEF; the same bits in an int32
buffer), so

  * `check()` finds every guard or pad word a kernel wrote, bit for bit, and says which buffer, which side of the payload
    and how many elements from the payload's edge;
  * `assert_defined(view)` finds every output element a kernel should have written and did not;
  * a read outside a payload whose value is USED turns the result into NaN, and the comparison with the reference
    fails.

What this cannot detect: a read outside the payload whose value is discarded (multiplied into a lane that is masked
off later, loaded and never used).  That needs an address sanitizer; the arena only sees what reaches memory or the
result.

float32 and int32 buffers, and the float64 / int64 ones some entry points write (the Gram matrices and patch counts
of cdl_nle_pca_gram*): `off` counts elements of the buffer's own type, so an 8-byte buffer at off = 1 sits on an 8-byte
aligned base that is not 16-byte aligned, which is all its element type asks for (two fill words read as one float64
are no NaN but 2.35e307, which no comparison with a reference survives either).  Byte-typed fragment buffers and
bf16 code buffers are not handed out: they are library-sized workspaces that must be 16-byte aligned anyway
(include/cdlnet_hip.h).
"""
import math

import torch

FILL_BITS = 0x7FC0BEEF          # a quiet NaN as float32; 2143338223 as int32
GUARD = 4096                    # words on each side
_ALIGN_WORDS = 64               # 256 bytes


class _Buf:
    __slots__ = ("name", "words", "start", "stop", "view", "is_output", "wpe")

    def __init__(self, name, words, start, stop, view, is_output, wpe=1):
        self.name, self.words, self.start, self.stop, self.view, self.is_output = name, words, start, stop, view, is_output
        self.wpe = wpe


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self.bufs = []

    def _carve(self, shape, off, dtype, name, is_output):
        if dtype not in (torch.float32, torch.int32, torch.float64, torch.int64):
            raise TypeError(f"arena buffers are float32 / int32 / float64 / int64, not {dtype}")
        shape = tuple(int(d) for d in shape)
        wpe = 2 if dtype in (torch.float64, torch.int64) else 1          # 4-byte words per element
        n = math.prod(shape) * wpe
        off = int(off) * wpe
        assert off >= 0 and n > 0
        total = GUARD + off + n + GUARD
        raw = torch.full((total + _ALIGN_WORDS,), FILL_BITS, dtype=torch.int32, device=self.device)
        skip = (-raw.data_ptr() % (4 * _ALIGN_WORDS)) // 4
        words = raw[skip:skip + total]
        assert words.data_ptr() % (4 * _ALIGN_WORDS) == 0
        start = GUARD + off
        view = words[start:start + n].view(dtype).view(shape)
        assert view.is_contiguous() and view.data_ptr() == words.data_ptr() + 4 * start
        name = name or f"buf{len(self.bufs)}"
        self.bufs.append(_Buf(name, words, start, start + n, view, is_output, wpe))
        return view

    def put(self, cpu_tensor, off, name=None):
        """An input: `cpu_tensor`'s values (float32 or int32) at element offset `off` between two guards."""
        t = cpu_tensor.detach().contiguous()
        view = self._carve(t.shape, off, t.dtype, name, False)
        view.copy_(t)
        return view

    def out(self, shape, off, dtype=torch.float32, name=None):
        """An output or work buffer: the payload holds the fill pattern until a kernel writes it."""
        return self._carve(shape, off, dtype, name, True)

    def _find(self, view):
        for b in self.bufs:
            if b.view.data_ptr() == view.data_ptr() and b.view.numel() == view.numel():
                return b
        raise KeyError("not a view this arena handed out")

    def words(self, view):
        """(int32 words of the whole region, payload start, payload stop in words): for tests of the arena itself."""
        b = self._find(view)
        return b.words, b.start, b.stop

    def violations(self):
        """["<buffer>: word <d> element(s) before|after the payload holds 0x........", ...] for every guard or pad
        word that no longer holds the fill pattern (at most 8 per side are spelled out)."""
        out = []
        for b in self.bufs:
            for side, seg, dist in (("before", b.words[:b.start], lambda i, b=b: b.start - i),
                                    ("after", b.words[b.stop:], lambda i: i + 1)):
                bad = (seg != FILL_BITS).nonzero().flatten()
                if bad.numel():
                    idx = bad[:8].tolist()
                    vals = seg[bad[:8]].tolist()
                    where = ", ".join(f"{dist(i)} ({v & 0xFFFFFFFF:#010x})" for i, v in zip(idx, vals))
                    out.append(f"{b.name}: {bad.numel()} word(s) {side} the payload overwritten, "
                               f"at distance(s) in elements from the payload's edge: {where}")
        return out

    def check(self):
        """Every guard and pad word still holds the fill pattern (compared as int32).  Call after a synchronize."""
        bad = self.violations()
        assert not bad, "guard words overwritten:\n  " + "\n  ".join(bad)

    def undefined(self, view):
        """Flat indices of the payload elements of `view` that still hold the fill pattern."""
        b = self._find(view)
        return (b.words[b.start:b.stop] == FILL_BITS).reshape(-1, b.wpe).all(1).nonzero().flatten()

    def assert_defined(self, view):
        """No element of an output payload still holds the fill pattern."""
        b = self._find(view)
        idx = self.undefined(view)
        assert idx.numel() == 0, (f"{b.name}: {idx.numel()} of {view.numel()} payload element(s) never written, "
                                  f"first at flat index {idx[:8].tolist()}")
