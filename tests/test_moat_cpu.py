"""The moat helper itself (tests/moat.py), on CPU tensors: it must report a planted write with the right offset, pass an
untouched buffer, hand back the payload bit for bit, and refuse moats that would change the payload's alignment."""
import pytest
import torch

from tests import moat

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _payload(dtype, n=1001):
    g = torch.Generator().manual_seed(n)
    t = torch.randn(n, 3, generator=g).to(dtype)
    t[0, 0] = float("nan")          # a NaN payload value must survive too
    t[1, 1] = float("-inf")
    return t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", ["nan", 0xFF])
def test_untouched_buffer_passes_and_view_round_trips(dtype, fill):
    t = _payload(dtype)
    view, guard = moat.embed(t, 1024, 512, fill)
    assert view.shape == t.shape and view.dtype == t.dtype and view.is_contiguous()
    assert view.data_ptr() % 64 == 0
    assert torch.equal(moat.bits(view), moat.bits(t))
    guard()
    assert guard.first_changed() is None
    # the moats really hold the pattern: NaN of the dtype, or 0xFF bytes
    flat = guard.flat
    assert flat.numel() == 1024 + t.numel() * t.element_size() + 512
    front = flat[:1024].view(dtype) if fill == "nan" else flat[:1024]
    assert bool(torch.isnan(front).all()) if fill == "nan" else bool((front == 0xFF).all())
    # writing the payload is no guard violation
    view.zero_()
    guard()


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_writes_are_reported_with_their_offsets(dtype):
    t = _payload(dtype)
    nbytes = t.numel() * t.element_size()
    pre, post = 1536, 1024
    # first guard word: 4 bytes starting `pre` bytes in front of the payload
    view, guard = moat.embed(t, pre, post, 0xFF)
    guard.flat[:4] = 0x55
    assert guard.first_changed() == -pre
    with pytest.raises(AssertionError, match=rf"offset -{pre} relative to the payload"):
        guard()
    # last guard word: its first byte is post - 4 bytes behind the payload's end
    view, guard = moat.embed(t, pre, post, "nan")
    guard.flat[-4:] = 0x55
    assert guard.first_changed() == nbytes + post - 4
    with pytest.raises(AssertionError, match=rf"offset {nbytes + post - 4} relative to the payload"):
        guard()
    # the words right next to the payload, and a single byte in the middle of a word
    view, guard = moat.embed(t, pre, post, "nan")
    guard.flat[pre - 1] = 0x01
    assert guard.first_changed() == -1
    view, guard = moat.embed(t, pre, post, 0xFF)
    guard.flat[pre + nbytes + 6] = 0x00
    assert guard.first_changed() == nbytes + 6
    # the earliest change wins
    guard.flat[7] = 0x00
    assert guard.first_changed() == 7 - pre


def test_payload_whose_size_is_no_multiple_of_4():
    idx = torch.arange(7, dtype=torch.uint8)          # a pooling index tensor
    view, guard = moat.embed(idx, 512, 512, 0xFF)
    assert torch.equal(view, idx)
    guard()
    guard.flat[512 + 7] = 0                           # the byte right behind it (inside an int32 word of the buffer)
    assert guard.first_changed() == 7
    h = torch.ones(5, dtype=torch.bfloat16)           # 10 bytes
    view, guard = moat.embed(h, 512, 512, "nan")
    guard()
    guard.flat[512 + 10] = 0x55
    assert guard.first_changed() == 10


@pytest.mark.parametrize("pre,post", [(100, 512), (512, 100), (0, 512), (512, 0), (513, 512), (512, 1023), (-512, 512)])
def test_misaligned_moats_are_rejected(pre, post):
    with pytest.raises(ValueError, match="multiples of 512"):
        moat.embed(torch.zeros(8), pre, post, 0xFF)


def test_bad_fill_and_layout_are_rejected():
    with pytest.raises(ValueError):
        moat.embed(torch.zeros(8, dtype=torch.uint8), 512, 512, "nan")     # no NaN in an integer type
    with pytest.raises(ValueError):
        moat.embed(torch.zeros(8), 512, 512, 0x1FF)
    with pytest.raises(ValueError):
        moat.embed(torch.zeros(8, 8).t(), 512, 512, 0xFF)


def test_moat_bytes():
    assert moat.moat_bytes() == 64 << 10
    assert moat.moat_bytes(3 * 4 + 3, 4) == 64 << 10
    # 2 * shift beyond 64 KiB: a conv of pad 3 on W = 1024, C = 4: shift (3 * 1024 + 3) * 4 floats
    shift = (3 * 1024 + 3) * 4
    b = moat.moat_bytes(shift, 4)
    assert b >= 2 * shift * 4 and b % 512 == 0 and b - 2 * shift * 4 < 512


def test_nan_like_and_bits():
    for dtype in DTYPES:
        assert bool(torch.isnan(moat.nan_like(torch.zeros(3, 5, dtype=dtype))).all())
    assert bool((moat.nan_like(torch.zeros(6, dtype=torch.uint8)) == 0xFF).all())
    a = torch.tensor([float("nan"), 0.0, -0.0])
    assert torch.equal(moat.bits(a), moat.bits(a.clone()))
    assert not torch.equal(moat.bits(a[1:2]), moat.bits(a[2:3]))          # +0 and -0 differ bit-wise


@pytest.mark.parametrize("poison", [0xFF, 0x00])
def test_moat_workspace_on_cpu(poison):
    class Ops:                      # the one thing moat_workspace needs of the ops module
        class Workspace:
            def __init__(self, device, nbytes=1 << 30):
                raise AssertionError("moat_workspace must not allocate the default workspace")

            @property
            def ptr(self):
                return self.buf.data_ptr()

    ws = moat.moat_workspace(Ops, 1000, poison, device="cpu", zero_head=True)
    assert ws.nbytes == 1000 and ws.buf.numel() == 1000 and ws.buf.dtype == torch.uint8 and ws.ptr == ws.buf.data_ptr()
    assert ws.head() == 0 and bool((ws.buf[4:] == poison).all())
    ws.guard()
    ws.buf.fill_(0x5A)              # a kernel may write all of its workspace ...
    ws.guard()
    ws.guard.flat[ws.guard.pre + 1000] = 0      # ... and not the byte behind it
    assert ws.guard.first_changed() == 1000
    with pytest.raises(ValueError):
        moat.moat_workspace(Ops, 16, 0xAA, device="cpu")
