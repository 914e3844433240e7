"""A numpy restatement of include/dcvc_hip_tnr_fuse.h and of tnr.TNR.rcp_table, written from their text (not from the
kernel or the module) on top of tests/tnr_ref.py: the per-reference weights, the blend in float32 operation by operation
in increasing j, the cells' sad / held -- and the stream rule of the look-ahead filter.  Integer work is int64."""
import numpy as np

from tests import tnr_ref as R

F32 = np.float32
FULL, MAX_REFS, RCP = R.FULL, 4, 1021


def rcp_table():
    """1021 float32: entry U is the float32 nearest the float64 quotient 1 / (256 + U)."""
    return (1.0 / (256.0 + np.arange(RCP, dtype=np.float64))).astype(F32)


def fuse(cur, refs, tab, P, rtab=None):
    """(out (3, H, W) float32, sad (hc, wc) int64, held (hc, wc) int64) of one dcvc_tnr_fuse with n = len(refs)."""
    assert 1 <= len(refs) <= MAX_REFS
    rtab = rcp_table() if rtab is None else np.asarray(rtab, dtype=F32)
    cur = np.asarray(cur, dtype=F32)
    acc = np.zeros(cur.shape, F32)
    U = np.zeros(cur.shape[1:], np.int64)
    d0 = None
    with np.errstate(invalid="ignore", over="ignore"):
        for ref in refs:
            ref = np.asarray(ref, dtype=F32)
            d, _, w = R.weights(cur, ref, tab, P)
            d0 = d if d0 is None else d0
            u = FULL - w                       # 0 .. 255
            t = ref - cur                      # (float32 operands: every operation below rounds to float32)
            t = t * u.astype(F32)[None]
            s = acc + t
            assert t.dtype == F32 and s.dtype == F32
            acc = np.where((u > 0)[None], s, acc)  # (a reference with u == 0 contributes nothing, a NaN in it included)
            U = U + u
        t = acc * rtab[U][None]
        blended = cur + t
        assert t.dtype == F32 and blended.dtype == F32
    out = np.where((U == 0)[None], cur, blended)
    return out, R.cell_sums(d0), R.cell_sums(U > 0)


def ahead_of(t, n_pics, intra, K):
    """The picture numbers an I picture t is fused with: the next min(K, pictures before the next I picture or the end)."""
    out = []
    for s in range(t + 1, min(t + 1 + K, n_pics)):
        if s in intra:
            break
        out.append(s)
    return out


def run(pics, tnr, intra, K, search=None):
    """[(the picture the codec is handed, sad, held, number of references, moved, zero)] of a stream: tnr is (T, floor, P),
    intra the picture numbers that are I pictures, each fused with the next pictures of its GOP, K at the most (none: passed
    through, everything 0); P pictures run through tnr_ref.step from the filtered I picture.  search = (R, lambda): every
    reference of an I picture is searched for from the I SOURCE and compensated (tests/me_ref.py) before the fusion, a P
    picture's reference is the compensated previous handed picture; moved is the number of cells with a nonzero vector and
    zero the sum of the SADs at the zero vector, of reference 0.  Without search both are 0."""
    from tests import me_ref as M

    T, floor, P = tnr
    tab, out = R.table(T, floor), []
    zeros = np.zeros(R.grid(*pics[0].shape[1:]), dtype=np.int64)

    def moved_onto(cur, ref):
        if search is None:
            return ref, 0, 0
        mv, _, zero = M.search(cur, ref, *search)
        return M.compensate(ref, mv), int((mv != 0).any(axis=2).sum()), int(zero.sum())

    for t, pic in enumerate(pics):
        if t in intra:
            ahead = ahead_of(t, len(pics), intra, K)
            if ahead:
                refs = [moved_onto(pic, pics[s]) for s in ahead]
                out.append(fuse(pic, [r[0] for r in refs], tab, P) + (len(ahead),) + refs[0][1:])
            else:
                out.append((np.asarray(pic, dtype=F32), zeros, zeros, 0, 0, 0))
        else:
            ref, moved, zero = moved_onto(pic, out[-1][0])
            out.append(R.step(pic, ref, tab, P) + (1, moved, zero))
    return out
