"""Guard regions ("moats") around kernel operands.

A kernel that reads a halo tap it should have masked, or whose buffer descriptor is a row too long, reads whatever lies next
to the tensor.  In a fresh process that is allocator slack, usually zero - exactly the padding value it should have produced.
embed() puts a tensor in the middle of one live allocation whose outer regions hold a known pattern: NaN for operands that are
read (a stray read poisons the result), the byte 0xFF for outputs and workspaces (a stray store changes a guard word).  Every
byte a wrong kernel could touch lies inside that allocation, so a failing case cannot fault.

No fixtures here: the tests import this module.
"""
import torch

ALIGN = 512                 # torch's device allocations are 512-byte aligned; pre / post keep the payload there
MIN_MOAT = 64 << 10

_NAN_WORD = {torch.float32: (4, 0x7FC00000), torch.bfloat16: (2, 0x7FC0), torch.float16: (2, 0x7E00)}


def moat_bytes(shift_elems=0, itemsize=4):
    """size of one moat for an operand whose buffer descriptor starts `shift_elems` elements before it:
    max(64 KiB, 2 * shift), rounded up to 512 bytes"""
    need = max(MIN_MOAT, 2 * int(shift_elems) * int(itemsize))
    return (need + ALIGN - 1) // ALIGN * ALIGN


def _pattern(fill, dtype):
    """-> the fill pattern as a list of byte values (its length divides 4)"""
    if fill == "nan":
        if dtype not in _NAN_WORD:
            raise ValueError(f"no NaN in {dtype}: fill such a tensor's moat with a byte")
        size, word = _NAN_WORD[dtype]
        return [(word >> (8 * i)) & 0xFF for i in range(size)]      # little endian
    if isinstance(fill, int) and 0 <= fill <= 0xFF:
        return [fill]
    raise ValueError(f"fill must be 'nan' or a byte value, got {fill!r}")


class Guard:
    """the two outer regions of one embed() buffer; calling it asserts that both still hold the fill pattern"""

    def __init__(self, flat, pre, nbytes, post, pattern, name):
        self.flat, self.pre, self.nbytes, self.post, self.pattern, self.name = flat, pre, nbytes, post, pattern, name

    def _expected(self, start, length):
        p = self.pattern
        reps = (length + len(p) - 1) // len(p) + 1
        phase = start % len(p)
        return torch.tensor(p, dtype=torch.uint8).repeat(reps)[phase:phase + length].to(self.flat.device)

    def first_changed(self):
        """byte offset, relative to the payload's first byte, of the first guard byte that changed (negative: in front of
        the payload; >= nbytes: behind it), or None"""
        word = int.from_bytes(bytes((self.pattern * 4)[:4]), "little", signed=True)
        for start, length in ((0, self.pre), (self.pre + self.nbytes, self.post)):
            # the region as int32 words (an unaligned head of up to 3 bytes behind an odd-sized payload goes bytewise)
            head = (-start) % 4
            body = self.flat[start + head:start + head + (length - head) // 4 * 4].view(torch.int32)
            if head == 0 and (length - head) % 4 == 0 and bool((body == word).all()):
                continue
            got = self.flat[start:start + length]
            bad = (got != self._expected(start, length)).nonzero()
            if bad.numel():
                return start + int(bad[0]) - self.pre
        return None

    def __call__(self):
        off = self.first_changed()
        assert off is None, (f"guard of {self.name} changed: first changed byte at offset {off} relative to the payload "
                             f"({self.nbytes} bytes, moats {self.pre} / {self.post})")


def embed(t, pre, post, fill, name="tensor"):
    """-> (view, guard): `t` copied into the middle of ONE flat buffer of pre + t.nbytes + post bytes on t's device, whose
    outer regions hold `fill` ('nan': NaN of t's dtype; or a byte value).  `view` is a contiguous tensor of t's shape and
    dtype; guard() asserts the outer regions are unchanged and names the first changed byte relative to the payload."""
    if pre <= 0 or post <= 0 or pre % ALIGN or post % ALIGN:
        raise ValueError(f"pre / post must be positive multiples of {ALIGN} bytes, got {pre} / {post}")
    if not t.is_contiguous():
        raise ValueError("embed() takes a contiguous tensor")
    pattern = _pattern(fill, t.dtype)
    nbytes = t.numel() * t.element_size()
    total = pre + nbytes + post
    flat = torch.empty(total, dtype=torch.uint8, device=t.device)
    if len(pattern) == 1:
        flat.fill_(pattern[0])
    else:
        unit = torch.tensor(pattern, dtype=torch.uint8, device=t.device)
        flat.view(total // len(pattern), len(pattern)).copy_(unit.expand(total // len(pattern), len(pattern)))
    view = flat[pre:pre + nbytes].view(t.dtype).view(t.shape)
    view.copy_(t)
    return view, Guard(flat, pre, nbytes, post, pattern, name)


def nan_like(t):
    """a tensor like t filled with NaN (floating types) or the byte 0xFF (integer types): the pre-fill of an output payload"""
    if t.dtype in _NAN_WORD:
        return torch.full_like(t, float("nan"))
    return torch.full_like(t.view(torch.uint8), 0xFF).view(t.dtype).view(t.shape)


def bits(t):
    """t's storage as integers, for bit-exact comparison (NaN payloads included)"""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def moat_workspace(ops, nbytes, poison, device="cuda", zero_head=False, moat=MIN_MOAT):
    """-> an ops.Workspace whose .buf is a moated view of exactly `nbytes` bytes, every byte `poison` (0xFF or 0x00), the
    moats 0xFF; .guard() checks them.  zero_head: the first 4 bytes are zeroed after poisoning (the entry points whose
    header says "first 4 bytes zero on first use"); .head() reads them back."""
    if poison not in (0xFF, 0x00):
        raise ValueError(f"poison must be 0xFF or 0x00, got {poison!r}")
    payload = torch.full((int(nbytes),), poison, dtype=torch.uint8, device=device)
    view, guard = embed(payload, moat, moat, 0xFF, name=f"workspace[{nbytes}]")
    if zero_head:
        view[:4] = 0
    ws = ops.Workspace.__new__(ops.Workspace)
    ws.buf, ws.nbytes, ws.guard = view, int(nbytes), guard
    ws.head = lambda: int(view[:4].view(torch.int32)[0])
    return ws
