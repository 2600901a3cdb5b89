"""Keyframe covisibility: one bit per (keyframe, Gaussian), kept on the device (include/gsraster.h, csrc/covis.hip).

The reference draws its training views blindly (lioOptimization.cpp:1573-1641).  A host that refines poses and prunes
floaters wants to know which keyframes see the same Gaussians (when to add a keyframe, which one to retire, which
history view constrains the current one) and how many keyframes see each Gaussian (freshly inserted rows that fewer than
n keyframes observe are the floaters).  Both exist in the project only as one `radii` tensor per forward; here they are
packed into bitsets in one launch per keyframe, queried with integer kernels, and they follow the model through
`GrowableGaussians.prune`.  Everything is integer arithmetic: exact and bitwise reproducible.

A visibility row is int64 words, little-endian in the bit order: bit i % 64 of word i // 64 belongs to model row i.
Which keyframes to choose, with which thresholds, and when to prune stays with the caller.
"""
import ctypes as C

import torch

from ._capi import _check, _stream, lib


def _words(P):
    return (int(P) + 63) // 64


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _slab(t, what):
    """(tensor, rows, pitch in words) of a [rows, >= words] int64 device tensor whose rows are contiguous (a view with a
    row stride is a slab with a pitch); a 1-D tensor is one row."""
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if not (t.is_cuda and t.dtype == torch.int64 and t.dim() == 2 and (t.size(1) <= 1 or t.stride(1) == 1)):
        raise ValueError("%s: expected an int64 device tensor [rows, words] with contiguous rows" % what)
    pitch = int(t.stride(0)) if t.size(0) > 1 else max(int(t.stride(0)), int(t.size(1)))
    return t, int(t.size(0)), pitch


def _source(src):
    """(radii, mask, P): an int32 tensor is a forward's radii, a bool / uint8 tensor a mask (mark_visible's)."""
    src = src.reshape(-1)
    if not src.is_cuda or not src.is_contiguous():
        raise ValueError("visibility_pack: expected a contiguous device tensor")
    if src.dtype == torch.int32:
        return src, None, int(src.numel())
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)
    if src.dtype != torch.uint8:
        raise ValueError("visibility_pack: int32 radii or a bool / uint8 mask, not %s" % src.dtype)
    return None, src, int(src.numel())


def visibility_pack(src, out=None, words=None):
    """One keyframe's visibility row in one launch (gsr_visibility_pack).  src: the forward's `radii` ([P] int32; seen =
    radii > 0) or a bool / uint8 mask as `mark_visible` returns it.  out: a contiguous int64 device tensor of at least
    `words` entries to write (a row of a slab), None = a new one; words: default all of `out`, or ceil(P / 64).  All
    `words` words are written, bits at and beyond P are zero.  Returns out[:words]."""
    radii, mask, P = _source(src)
    if words is None:
        words = int(out.numel()) if out is not None else _words(P)
    if out is None:
        out = torch.empty(int(words), dtype=torch.int64, device=src.device)
    if not (out.is_cuda and out.dtype == torch.int64 and out.dim() == 1 and out.is_contiguous() and out.numel() >= words):
        raise ValueError("visibility_pack: out is a contiguous int64 device tensor of at least `words` entries")
    _check(lib().gsr_visibility_pack(P, _vp(radii), _vp(mask), _vp(out), int(words), _stream()))
    return out[:words]


def covisibility(q_bits, k_bits=None, words=None, counts=True, out=None):
    """inter[q, k] = the number of Gaussians that query row q and keyframe row k both see (gsr_covisibility), one launch.
    q_bits / k_bits: int64 device tensors [Q, .] / [K, .] with contiguous rows (a 1-D tensor is one row; k_bits None =
    q_bits: the full matrix, whose diagonal is the counts); words: how many words of each row count, default all that
    both hold.  Returns (inter [Q, K] int32, q_count [Q], k_count [K]), the counts None with counts=False.  out: three
    contiguous int32 tensors (the last two may be None) to write instead of new ones."""
    q, Q, qp = _slab(q_bits, "covisibility")
    k, K, kp = (q, Q, qp) if k_bits is None else _slab(k_bits, "covisibility")
    if words is None:
        words = min(int(q.size(1)), int(k.size(1)))
    if words > q.size(1) or words > k.size(1):
        raise ValueError("covisibility: a row holds fewer than %d words" % words)
    i32 = dict(dtype=torch.int32, device=q.device)
    if out is None:
        out = (torch.empty((Q, K), **i32), torch.empty(Q, **i32) if counts else None,
               torch.empty(K, **i32) if counts else None)
    inter, qc, kc = out
    for t, n in ((inter, Q * K), (qc, Q), (kc, K)):
        if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
            raise ValueError("covisibility: outputs are contiguous int32 device tensors [Q, K], [Q], [K]")
    _check(lib().gsr_covisibility(Q, _vp(q), qp, K, _vp(k), kp, int(words), _vp(inter), _vp(qc), _vp(kc), _stream()))
    return inter, qc, kc


def observation_count(bits, P, first_row=0, min_count=0, want_count=True, want_drop=False, out=None):
    """How many of the K rows of `bits` ([K, >= ceil(P / 64)] int64) see each of the P model rows (gsr_observation_count),
    one launch.  Returns (count [P] int32 or None, drop [P] uint8 or None) with drop[i] = (i >= first_row and count[i] <
    min_count): the shape `GrowableGaussians.prune(drop=)` takes.  out: (count, drop) tensors to write instead."""
    b, K, pitch = _slab(bits, "observation_count")
    P = int(P)
    if b.size(1) < _words(P):
        raise ValueError("observation_count: the rows hold fewer than %d words" % _words(P))
    if out is None:
        out = (torch.empty(P, dtype=torch.int32, device=b.device) if want_count else None,
               torch.empty(P, dtype=torch.uint8, device=b.device) if want_drop else None)
    count, drop = out
    if count is not None and not (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous() and
                                  count.numel() == P):
        raise ValueError("observation_count: count is a contiguous int32 device tensor [P]")
    if drop is not None and not (drop.is_cuda and drop.dtype == torch.uint8 and drop.is_contiguous() and
                                 drop.numel() == P):
        raise ValueError("observation_count: drop is a contiguous uint8 device tensor [P]")
    _check(lib().gsr_observation_count(K, _vp(b), pitch, P, int(first_row), int(min_count), _vp(count), _vp(drop),
                                       _stream()))
    return count, drop


def visibility_remap(src, reasons, row_map, dst=None, dst_words=None):
    """The rows of `src` ([K, >= ceil(P / 64)] int64) after a stable compaction (gsr_visibility_remap), one launch, out of
    place: bit row_map[i] of a destination row = bit i of its source row where reasons[i] == 0, every other bit of its
    dst_words words zero.  reasons [P] uint8 and row_map [P + 1] int32 on the device, as `_capi.prune_mark` returns them.
    dst: a [K, >= dst_words] int64 tensor with contiguous rows, None = a new [K, dst_words] one; dst_words: default
    ceil(P / 64), which always suffices.  Returns dst."""
    s, K, sp = _slab(src, "visibility_remap")
    P = int(reasons.numel())
    if not (reasons.is_cuda and reasons.dtype == torch.uint8 and reasons.is_contiguous()):
        raise ValueError("visibility_remap: reasons is a contiguous uint8 device tensor [P]")
    if not (row_map.is_cuda and row_map.dtype == torch.int32 and row_map.is_contiguous() and row_map.numel() == P + 1):
        raise ValueError("visibility_remap: row_map is a contiguous int32 device tensor [P + 1]")
    if s.size(1) < _words(P):
        raise ValueError("visibility_remap: the source rows hold fewer than %d words" % _words(P))
    if dst_words is None:
        dst_words = int(dst.size(-1)) if dst is not None else _words(P)
    if dst is None:
        dst = torch.empty((K, int(dst_words)), dtype=torch.int64, device=s.device)
    d, Kd, dp = _slab(dst, "visibility_remap")
    if Kd != K or d.size(1) < dst_words:
        raise ValueError("visibility_remap: dst is [K, >= dst_words]")
    _check(lib().gsr_visibility_remap(K, _vp(s), sp, P, _vp(reasons), _vp(row_map), _vp(d), dp, int(dst_words),
                                      _stream()))
    return dst


def _f64(t):
    return torch.as_tensor(t).to(torch.float64)


def iou(inter, q_count, k_count):
    """inter / (q_count + k_count - inter) as float64 [Q, K]: the share of the Gaussians either view sees that both see.
    0 / 0 = 0."""
    i = _f64(inter)
    union = _f64(q_count).reshape(-1, 1) + _f64(k_count).reshape(1, -1) - i
    return torch.where(union > 0, i / union.clamp(min=1), torch.zeros_like(i))


def overlap_coefficient(inter, q_count, k_count):
    """inter / min(q_count, k_count) as float64 [Q, K]: 1 when one view sees a subset of the other.  0 / 0 = 0."""
    i = _f64(inter)
    least = torch.minimum(_f64(q_count).reshape(-1, 1), _f64(k_count).reshape(1, -1)).expand_as(i)
    return torch.where(least > 0, i / least.clamp(min=1), torch.zeros_like(i))


class KeyframeVisibility:
    """The visibility rows of the keyframes of one model as a [keyframes, words] int64 slab on the device.

    `rows` is the model's row count the records describe.  The slab grows by doubling in either direction (more
    keyframes, more model rows); old bits are kept and new bits are zero, so rows appended by `add_new_pointcloud` or
    `densify` keep the existing row numbers and older keyframes simply read 0 for them.  A prune renumbers rows:
    `GrowableGaussians.attach_visibility` makes `prune` call `remap`, otherwise the caller does."""

    def __init__(self, rows, keyframes=64, device="cuda"):
        self.device = torch.device(device)
        self.rows, self.n = int(rows), 0
        self._slab = torch.zeros((max(1, int(keyframes)), max(1, _words(rows))), dtype=torch.int64, device=self.device)
        self._scratch = None

    def __len__(self):
        return self.n

    @property
    def words(self):
        """words of a row that describe model rows: ceil(rows / 64) (the slab's pitch may be larger)"""
        return _words(self.rows)

    @property
    def bits(self):
        """[len, words] view of the recorded rows"""
        return self._slab[:self.n, :self.words]

    def _reserve(self, keyframes, rows):
        K, W = self._slab.shape
        K2, W2 = K, W
        while K2 < keyframes:
            K2 *= 2
        while W2 < _words(rows):
            W2 *= 2
        if (K2, W2) != (K, W):
            new = torch.zeros((K2, W2), dtype=torch.int64, device=self.device)
            new[:self.n, :W].copy_(self._slab[:self.n])
            self._slab = new
            self._scratch = None

    def record(self, radii_or_mask, slot=None):
        """Packs one forward's radii ([P] int32) or a visibility mask ([P] bool / uint8) into row `slot` (None = a new
        row behind the last) in one launch; returns the slot.  A source with more rows than any before grows the slab."""
        P = int(radii_or_mask.numel())
        slot = self.n if slot is None else int(slot)
        if not 0 <= slot <= self.n:
            raise IndexError("record: slot %d of %d keyframes" % (slot, self.n))
        self._reserve(slot + 1, max(P, self.rows))
        if P:
            visibility_pack(radii_or_mask, out=self._slab[slot])  # the whole pitch: no stale bit survives
        else:
            self._slab[slot].zero_()
        self.rows = max(self.rows, P)
        self.n = max(self.n, slot + 1)
        return slot

    def remove(self, slot):
        """Retires keyframe `slot`: the last row moves into the hole (its slot number becomes `slot`)."""
        slot = int(slot)
        if not 0 <= slot < self.n:
            raise IndexError("remove: slot %d of %d keyframes" % (slot, self.n))
        if slot != self.n - 1:
            self._slab[slot].copy_(self._slab[self.n - 1])
        self.n -= 1

    def _need_records(self, what):
        if self.n == 0 or self.rows == 0:
            raise ValueError("%s: no keyframe is recorded" % what)

    def overlap(self, query=None):
        """(inter [Q, K] int32, q_count [Q], k_count [K]) against the K recorded keyframes.  query: None = all recorded
        rows (the full matrix), a slot number, or a radii / mask tensor, which is packed into a scratch row and not
        recorded."""
        self._need_records("overlap")
        k = self._slab[:self.n]
        if query is None:
            return covisibility(k, None, words=self.words)
        if isinstance(query, torch.Tensor):
            if query.numel() > self.rows:
                raise ValueError("overlap: the query has %d rows, the records %d" % (query.numel(), self.rows))
            if self._scratch is None:
                self._scratch = torch.empty(self._slab.size(1), dtype=torch.int64, device=self.device)
            q = visibility_pack(query, out=self._scratch)
        else:
            slot = int(query)
            if not 0 <= slot < self.n:
                raise IndexError("overlap: slot %d of %d keyframes" % (slot, self.n))
            q = self._slab[slot]
        return covisibility(q, k, words=self.words)

    def observation_count(self, P=None):
        """[P] int32: how many recorded keyframes see each model row (P: default `rows`; rows beyond the records count 0)."""
        P = self.rows if P is None else int(P)
        self._need_records("observation_count")
        self._reserve(self.n, P)
        return observation_count(self._slab[:self.n], P)[0]

    def unobserved(self, min_count, first_row=0, P=None):
        """[P] uint8: 1 for the rows from `first_row` on that fewer than `min_count` keyframes see -- the mask
        `GrowableGaussians.prune(drop=)` takes."""
        P = self.rows if P is None else int(P)
        self._need_records("unobserved")
        self._reserve(self.n, P)
        return observation_count(self._slab[:self.n], P, first_row, min_count, want_count=False, want_drop=True)[1]

    def remap(self, reasons, row_map, rows_after=None):
        """Follows a stable compaction of the model's rows: reasons [P] uint8 on the device and row_map [P + 1] int32 as
        `prune` returns them (a host row_map is uploaded).  rows_after: P' when the caller has it (else row_map[P] is
        fetched).  One launch, out of place; the old slab is released."""
        P = int(reasons.numel())
        if row_map.numel() != P + 1:
            raise ValueError("remap: row_map has %d entries, reasons %d" % (row_map.numel(), P))
        if rows_after is None:
            rows_after = int(row_map[P])
        if self.n and P:
            self._reserve(self.n, P)
            row_map = row_map.to(device=self.device, dtype=torch.int32).contiguous()
            new = torch.empty_like(self._slab)
            visibility_remap(self._slab[:self.n], reasons.to(self.device), row_map, dst=new[:self.n])
            self._slab = new
        self.rows = int(rows_after)
