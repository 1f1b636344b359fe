"""numpy restatement of the batch-mixing contract (include/wsdl_hip.h "batch mixing"): the ClassMix class selection
with Python integers modulo 2^64, the three mask sources, and the apply by fancy indexing.  Nothing here is approximate: the
device must give these arrays bit for bit.

A batch has B items with planes of H x W.  ``partner`` int32 (B,): item b is mixed with item ``partner[b]``; a value outside
``[0, B)`` leaves item b unmixed (mask 0 everywhere).  ``M[b,y,x]`` in {0,1}, 1 = "take the partner's pixel":
  "box"    ``boxes`` int32 (B,R,4), rows (y0, x0, y1, x1) half-open: M = 1 inside the union; empty boxes contribute nothing;
           coordinates outside the image clip implicitly.
  "class"  M = 1 iff ``class_labels[partner[b],y,x]`` is in the 64-bit set ``sel[partner[b]]``; a label outside [0, 64) never is.
  "mask"   M = ``mask[b] != 0``.
``invert`` flips M for mixed items only.  out_T[b,...,y,x] = M[b,y,x] ? T[partner[b],...,y,x] : T[b,...,y,x].
"""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def fmix(z):
    """The splitmix64 finaliser on a Python int in [0, 2^64)."""
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def key(seed, c):
    """key(c) = fmix(uint64(seed) + (c + 1) * GOLDEN) modulo 2^64; ``seed`` any Python int (an int64 wraps to its uint64)."""
    return fmix(((int(seed) & MASK64) + (c + 1) * GOLDEN) & MASK64)


def present_classes(labels_i, num_classes, candidates=None):
    """The candidates c in [0, num_classes) for which some pixel of the label map equals c, ascending."""
    have = set(int(v) for v in np.unique(labels_i))
    cands = range(num_classes) if candidates is None else candidates
    return sorted(c for c in set(cands) if 0 <= c < num_classes and c in have)


def select_classes(present, seed):
    """The k = ceil(n / 2) classes of ``present`` with the smallest (key, c): class c is selected iff fewer than k present
    classes come before it."""
    k = (len(present) + 1) // 2
    keys = {c: key(seed, c) for c in present}
    return [c for c in present if sum((keys[d], d) < (keys[c], c) for d in present) < k]


def word(classes):
    w = 0
    for c in classes:
        w |= 1 << c
    return w


def as_int64(words):
    return np.array([w & MASK64 for w in words], dtype=np.uint64).view(np.int64)


def class_select(class_labels, num_classes, seeds, candidates=None):
    """-> (sel, present): int64 (B,) arrays of 64-bit sets."""
    sel, pres = [], []
    for lab, seed in zip(class_labels, seeds):
        p = present_classes(lab, num_classes, candidates)
        pres.append(word(p))
        sel.append(word(select_classes(p, int(seed))))
    return as_int64(sel), as_int64(pres)


def mix_mask(kind, partner, shape, *, boxes=None, class_labels=None, sel=None, mask=None, invert=False):
    """M as a uint8 (B,H,W) array."""
    B, H, W = shape
    M = np.zeros((B, H, W), dtype=bool)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    for b in range(B):
        pb = int(partner[b])
        if not 0 <= pb < B:
            continue                                    # unmixed: 0 everywhere, whatever ``invert`` says
        if kind == "box":
            for y0, x0, y1, x1 in np.asarray(boxes[b]).astype(np.int64):
                M[b] |= (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
        elif kind == "class":
            chosen = int(sel[pb]) & MASK64
            lab = class_labels[pb]
            table = np.array([(chosen >> c) & 1 for c in range(64)], dtype=bool)
            ok = (lab >= 0) & (lab < 64)
            M[b] = ok & table[np.where(ok, lab, 0)]
        elif kind == "mask":
            M[b] = mask[b] != 0
        else:
            raise ValueError(kind)
        if invert:
            M[b] = ~M[b]
    return M.astype(np.uint8)


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def apply(M, partner, T):
    """out_T of one tensor (B,H,W) or (B,C,H,W), as a bit copy (float arrays travel as integer words)."""
    T = np.ascontiguousarray(T)
    bits = _bits(T)
    out = bits.copy()
    B = T.shape[0]
    for b in range(B):
        pb = int(partner[b])
        if 0 <= pb < B:
            m = M[b].astype(bool)
            out[b][..., m] = bits[pb][..., m]
    return out.view(T.dtype)


def mix_batch(images, labels, partner, *, kind, boxes=None, class_labels=None, sel=None, mask=None, invert=False, pixel_weight=None,
              scores=None):
    """-> dict of every result of ``ops.mix_batch``: images, labels, pixel_weight, scores (None where not given), mask (uint8),
    mixed_count (int64 (B,))."""
    B, H, W = labels.shape
    M = mix_mask(kind, partner, (B, H, W), boxes=boxes, class_labels=class_labels, sel=sel, mask=mask, invert=invert)
    res = {"mask": M, "mixed_count": M.reshape(B, -1).sum(axis=1).astype(np.int64)}
    for name, T in (("images", images), ("labels", labels), ("pixel_weight", pixel_weight), ("scores", scores)):
        res[name] = None if T is None else apply(M, partner, T)
    return res
