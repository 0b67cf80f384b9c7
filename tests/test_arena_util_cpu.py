"""The guard-band arena of the GPU parity tests, checked on its own on a CPU arena."""
import pytest
import torch

import arena_util
from arena_util import Arena, FILL_BITS, GUARD


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_layout_alignment_and_fill(off):
    a = Arena("cpu")
    x = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    v = a.put(x, off, "x")
    o = a.out((2, 7), off, name="o")
    m = a.out((4,), off, torch.int32, "m")
    for t in (v, o, m):
        words, start, stop = a.words(t)
        assert words.data_ptr() % 256 == 0 and start == GUARD + off and stop == start + t.numel()
        assert t.data_ptr() % 256 == (4 * off) % 256 and t.is_contiguous()
        assert words.numel() - stop >= GUARD
    assert torch.equal(v, x)
    assert bool(torch.isnan(o).all()) and bool((o.view(torch.int32) == FILL_BITS).all())
    assert bool((m == FILL_BITS).all())
    a.check()
    assert a.undefined(o).numel() == 14
    with pytest.raises(AssertionError):
        a.assert_defined(o)
    a.assert_defined(v)


def test_check_names_a_word_before_after_and_an_unwritten_one():
    a = Arena("cpu")
    ok = a.put(torch.ones(6), 1, "ok")
    o = a.out((3, 4), 2, name="victim")
    o.fill_(1.0)
    a.check()
    a.assert_defined(o)
    words, start, stop = a.words(o)

    words[start - 1] = 0                                     # the pad word right before the payload
    msg = "\n".join(a.violations())
    assert "victim" in msg and "before" in msg and "edge: 1 (0x00000000)" in msg and "ok" not in msg
    with pytest.raises(AssertionError, match="victim: 1 word.s. before"):
        a.check()
    words[start - 1] = FILL_BITS
    a.check()

    words[stop + 2] = 0x3F800000                             # the third word after it
    msg = "\n".join(a.violations())
    assert "victim" in msg and "after" in msg and "edge: 3 (0x3f800000)" in msg and "before" not in msg
    with pytest.raises(AssertionError, match="victim: 1 word.s. after"):
        a.check()
    words[stop + 2] = FILL_BITS
    a.check()

    o.view(-1)[7] = torch.tensor(FILL_BITS, dtype=torch.int32).view(torch.float32)     # one element left unwritten
    assert a.undefined(o).tolist() == [7]
    with pytest.raises(AssertionError, match=r"victim: 1 of 12 payload element.s. never written.*\[7\]"):
        a.assert_defined(o)
    a.assert_defined(ok)
    a.check()                                                # the payload is not the guard's business


@pytest.mark.parametrize("off", [0, 1, 2])
def test_eight_byte_types_count_offsets_in_their_own_elements(off):
    a = Arena("cpu")
    g = a.out((3, 3), off, torch.float64, "gram")
    n = a.put(torch.arange(4, dtype=torch.int64), off, "count")
    for t in (g, n):
        words, start, stop = a.words(t)
        assert start == GUARD + 2 * off and stop == start + 2 * t.numel()
        assert t.data_ptr() % 8 == 0 and t.data_ptr() % 256 == (8 * off) % 256
    assert bool((g > 1e300).all()) and n.tolist() == [0, 1, 2, 3]       # two fill words as one float64: 2.35e307
    assert a.undefined(g).numel() == 9
    g.fill_(2.0)
    a.assert_defined(g)
    g.view(-1)[4] = float("nan")                             # a NaN the kernel computed is not the fill pattern
    a.assert_defined(g)
    words, start, stop = a.words(g)
    words[start + 8] = FILL_BITS
    a.assert_defined(g)                                      # half an element is not an unwritten element
    words[start + 9] = FILL_BITS
    assert a.undefined(g).tolist() == [4]
    words[stop] = 1
    with pytest.raises(AssertionError, match="gram: 1 word.s. after"):
        a.check()


def test_other_types_are_refused():
    for dt in (torch.float16, torch.uint8, torch.bfloat16):
        with pytest.raises(TypeError):
            Arena("cpu").out((4,), 0, dt)
    assert arena_util.GUARD >= 4096
