"""Placement of test tensors (GPU tests): every tensor is a view at a chosen byte offset (0/4/8/12) inside its own, larger
allocation whose other floats hold a NaN pattern no kernel produces -- guards in front of and behind the view, and the
prefill of outputs not yet written.  Shared by test_gpu_optim_ref64.py and test_gpu_sh_layouts.py."""
import torch

PAT = 0x7FC0DEAD   # a quiet NaN no kernel produces: guards and not-yet-written outputs
LEAD = 4           # guard floats in front of a view (16 bytes: keeps the base alignment), at least 9 behind


# ---- placement: every tensor is a view at a chosen byte offset inside its own, larger, guarded allocation ----------
class Arena:
    def __init__(self, dev, offset_of):
        self.dev, self.offset_of, self.t, self.buf, self.span = dev, offset_of, {}, {}, {}

    def put(self, name, src=None, shape=None):
        shape = tuple(src.shape) if src is not None else tuple(shape)
        n = 1
        for s in shape:
            n *= s
        off = self.offset_of(name, len(self.t))
        assert off in (0, 4, 8, 12)
        buf = torch.full((n + 16,), PAT, dtype=torch.int32, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        start = LEAD + off // 4
        view = buf.view(torch.float32)[start:start + n].view(shape)
        if src is not None:
            view.copy_(src)
        assert n == 0 or view.data_ptr() % 16 == off
        self.t[name], self.buf[name], self.span[name] = view, buf, (start, n)
        return view

    def ptr(self, name):
        t = self.t[name]
        return t.data_ptr() if t.numel() else None

    def guards_intact(self):
        for name, buf in self.buf.items():
            start, n = self.span[name]
            if not (bool((buf[:start] == PAT).all()) and bool((buf[start + n:] == PAT).all())):
                return name
        return None


def offsets(mode):
    """all tensors at one offset ("a0" "a4" "a8" "a12"), cycling through 0/4/8/12 ("mix"), or one parameter group
    (its parameter and both moments) at 8 bytes and everything else aligned ("only:<group>")."""
    if mode == "mix":
        return lambda name, i: (0, 4, 8, 12)[i % 4]
    if mode.startswith("only:"):
        grp = mode[5:]
        return lambda name, i: 8 if name in ("p." + grp, "m." + grp, "v." + grp) else 0
    return lambda name, i: int(mode[1:])
