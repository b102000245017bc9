"""Token-level scoring: the definition (include/asr_hip.h: asr_edit_align), in plain Python and numpy integers.

For a reference r[0..m) and a hypothesis h[0..n) of token ids:
    D[i][0] = i, D[0][j] = j
    D[i][j] = min(D[i-1][j-1] + (r[i-1] != h[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
The direction of a cell with i, j > 0 is the first that applies of
    DIAG   D[i-1][j-1] + (r[i-1] != h[j-1]) == D[i][j]
    UP     D[i-1][j] + 1 == D[i][j]                        (r[i-1] is deleted)
    LEFT   otherwise                                       (h[j-1] is inserted)
Row 0 is all LEFT, column 0 all UP.  The alignment is the walk from (m, n) to (0, 0) along the directions, reported in forward order as
(op, ref_pos, hyp_pos), ref_pos = -1 for an insertion and hyp_pos = -1 for a deletion.  The tie order is part of the definition: the
distance does not depend on it, the split into substitutions, deletions and insertions does."""
import numpy as np

COR, SUB, DEL, INS = 0, 1, 2, 3
DIAG, UP, LEFT = 0, 1, 2


def table(ref, hyp):
    """D as an (m + 1, n + 1) int64 array.  Row by row; the dependence along a row is the running minimum of t[k] - k."""
    r, h = np.asarray(ref, dtype=np.int64).reshape(-1), np.asarray(hyp, dtype=np.int64).reshape(-1)
    m, n = r.shape[0], h.shape[0]
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    D[0] = np.arange(n + 1)
    col = np.arange(n + 1)
    for i in range(1, m + 1):
        t = np.empty(n + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (r[i - 1] != h))
        D[i] = np.minimum.accumulate(t - col) + col
    return D


def directions(ref, hyp, D=None):
    """(m + 1, n + 1) array of DIAG / UP / LEFT."""
    r, h = np.asarray(ref, dtype=np.int64).reshape(-1), np.asarray(hyp, dtype=np.int64).reshape(-1)
    D = table(r, h) if D is None else D
    m, n = r.shape[0], h.shape[0]
    d = np.full((m + 1, n + 1), LEFT, dtype=np.int8)
    d[:, 0] = UP
    d[0, :] = LEFT
    if m and n:
        sub = (r[:, None] != h[None, :]).astype(np.int64)
        diag = D[:-1, :-1] + sub == D[1:, 1:]
        up = D[:-1, 1:] + 1 == D[1:, 1:]
        d[1:, 1:] = np.where(diag, DIAG, np.where(up, UP, LEFT))
    return d


def align(ref, hyp):
    """{"distance", "cor", "sub", "del", "ins", "ops": [(op, ref_pos, hyp_pos), ...]} of one pair."""
    r, h = [int(x) for x in ref], [int(x) for x in hyp]
    D = table(r, h)
    d = directions(r, h, D)
    i, j = len(r), len(h)
    ops = []
    while i > 0 or j > 0:
        k = int(d[i, j])
        if k == DIAG:
            ops.append((COR if r[i - 1] == h[j - 1] else SUB, i - 1, j - 1))
            i, j = i - 1, j - 1
        elif k == UP:
            ops.append((DEL, i - 1, -1))
            i -= 1
        else:
            ops.append((INS, -1, j - 1))
            j -= 1
    ops.reverse()
    n = [sum(1 for o in ops if o[0] == c) for c in (COR, SUB, DEL, INS)]
    return {"distance": int(D[len(r), len(h)]), "cor": n[0], "sub": n[1], "del": n[2], "ins": n[3], "ops": ops}

