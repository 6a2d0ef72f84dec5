"""kdb_align_traceback restated from the definition in include/kdbhip.h (test infrastructure: the product never imports this).

THE WALK.  The recurrence, its tie rules and the best cell are alignment_cases.py's.  Start at the best cell in state H.
  state H at (i, j): if H took the diagonal term (the first of [diagonal, E, F] that reaches its value): emit `=` if Q[i] = R[j] and both
    are ACGT, else X; if H(i - 1, j - 1) = 0 or there is no such cell, stop; otherwise go on in state H at (i - 1, j - 1).  If H took E:
    state E at (i, j), nothing emitted.  Otherwise state F at (i, j), nothing emitted.
  state E at (i, j): emit D.  If H(i, j - 1) + gap_open >= E(i, j - 1) + gap_extend go on in state H at (i, j - 1), else in state E there.
  state F at (i, j): emit I.  If H(i - 1, j) + gap_open >= F(i - 1, j) + gap_extend go on in state H at (i - 1, j), else in state F there.
The emitted ops are reversed and run-length encoded, equal neighbours merged; a run is (len << 4) | op, I = 1, D = 2, `=` = 7, X = 8.

trace() keeps, beside alignment_cases.banded's rows, what every in-band cell decided -- where its H came from, whether its E and its F
opened -- and walks those tables; the cell the walk stops at is the origin it reports.  trace_full() is written on its own: full
(m + 1) x (n + 1) matrices of values alone, as alignment_cases.unbanded fills them, and a walk that decides every step by comparing
values.  trace() must equal it when the band covers the matrix.
"""
import alignment_cases as ac

NINF = ac.NINF
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
CHAR = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}


def encode(ops_backwards):
    """the ops as the walk emits them, last first -> the runs from the origin to the end"""
    runs = []
    for op in reversed(ops_backwards):
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return [(n << 4) | op for n, op in runs]


def text(runs):
    return "".join("{0}{1}".format(int(r) >> 4, CHAR[int(r) & 15]) for r in runs)


def trace(q, r, d, band, strand=0, match=3, mismatch=-1, gap_open=-10, gap_extend=-1):
    """-> ((score, qstart, qend, rstart, rend), runs).  The rows are alignment_cases.banded's; came[(i, j)] = 0 the diagonal from H = 0 or
    from no cell, 1 the diagonal, 2 E, 3 F; e_opens / f_opens[(i, j)]: E(i, j) / F(i, j) took the H + gap_open term."""
    Q, R = ac.orient(q, strand), bytes(r)
    m, n, W = len(Q), len(R), 2 * band + 1
    Hp, Fp = [0] * (W + 2), [NINF] * (W + 2)
    came, e_opens, f_opens = {}, {}, {}
    best, best_cell = 0, None
    for i in range(m):
        H, E, F = [0] * (W + 2), [NINF] * (W + 2), [NINF] * (W + 2)
        for c in range(W):
            j = i + d - band + c
            if j < 0 or j >= n:
                continue
            x = c + 1
            open_e, ext_e = H[x - 1] + gap_open, E[x - 1] + gap_extend
            open_f, ext_f = Hp[x + 1] + gap_open, Fp[x + 1] + gap_extend
            e, f = max(open_e, ext_e), max(open_f, ext_f)
            dg = Hp[x] + ac._s(Q[i], R[j], match, mismatch)
            h = max(0, dg, e, f)
            H[x], E[x], F[x] = h, e, f
            came[(i, j)] = (0 if Hp[x] == 0 else 1) if dg == h else 2 if e == h else 3
            e_opens[(i, j)], f_opens[(i, j)] = open_e >= ext_e, open_f >= ext_f
            if h > best:                                                      # (rows ascend and, inside a row, columns: the first cell to reach a score keeps it)
                best, best_cell = h, (i, j)
        Hp, Fp = H, F
    if best == 0:
        return (0, 0, 0, 0, 0), []
    (i, j), state, ops = best_cell, "H", []
    while True:
        if state == "H":
            how = came[(i, j)]
            if how <= 1:
                ops.append(OP_EQ if Q[i] == R[j] and Q[i] in b"ACGT" else OP_X)
                if how == 0:
                    break
                i, j = i - 1, j - 1
            else:
                state = "E" if how == 2 else "F"
        elif state == "E":
            ops.append(OP_D)
            state = "H" if e_opens[(i, j)] else "E"
            j -= 1
        else:
            ops.append(OP_I)
            state = "H" if f_opens[(i, j)] else "F"
            i -= 1
    return (best, i, best_cell[0] + 1, j, best_cell[1] + 1), encode(ops)


def trace_full(Q, R, match=3, mismatch=-1, gap_open=-10, gap_extend=-1):
    """The whole matrix, values alone, and a walk that compares values -> ((score, qstart, qend, rstart, rend), runs) of the oriented
    query Q.  Row 0 and column 0 are the border: H = 0, E = F = -infinity."""
    Q, R = bytes(Q), bytes(R)
    m, n = len(Q), len(R)
    grid = lambda v: [[v] * (n + 1) for _ in range(m + 1)]
    H, E, F = grid(0), grid(NINF), grid(NINF)
    s = lambda a, b: match if Q[a - 1] == R[b - 1] and Q[a - 1] in b"ACGT" else mismatch
    for a in range(1, m + 1):
        for b in range(1, n + 1):
            E[a][b] = max(H[a][b - 1] + gap_open, E[a][b - 1] + gap_extend)
            F[a][b] = max(H[a - 1][b] + gap_open, F[a - 1][b] + gap_extend)
            H[a][b] = max(0, H[a - 1][b - 1] + s(a, b), E[a][b], F[a][b])
    top = max(max(row) for row in H)
    if top == 0:
        return (0, 0, 0, 0, 0), []
    a, b = end = min((a, b) for a in range(m + 1) for b in range(n + 1) if H[a][b] == top)
    state, ops = "H", []
    while True:
        if state == "H":
            if H[a][b] == H[a - 1][b - 1] + s(a, b):
                ops.append(OP_EQ if s(a, b) == match and Q[a - 1] == R[b - 1] and Q[a - 1] in b"ACGT" else OP_X)
                a, b = a - 1, b - 1
                if H[a][b] == 0:
                    break
            elif H[a][b] == E[a][b]:
                state = "E"
            else:
                state = "F"
        elif state == "E":
            ops.append(OP_D)
            state = "H" if H[a][b - 1] + gap_open >= E[a][b - 1] + gap_extend else "E"
            b -= 1
        else:
            ops.append(OP_I)
            state = "H" if H[a - 1][b] + gap_open >= F[a - 1][b] + gap_extend else "F"
            a -= 1
    return (top, a, end[0], b, end[1]), encode(ops)


def spans(runs):
    """-> (query residues, reference residues) the runs consume"""
    q = sum(int(r) >> 4 for r in runs if int(r) & 15 in (OP_EQ, OP_X, OP_I))
    return q, sum(int(r) >> 4 for r in runs if int(r) & 15 in (OP_EQ, OP_X, OP_D))


def rescore(runs, match=3, mismatch=-1, gap_open=-10, gap_extend=-1):
    """the score the runs stand for: match per =, mismatch per X, gap_open + (len - 1) max(gap_open, gap_extend) per gap run (where
    gap_open > gap_extend every residue of a gap is an opening, and abutting gaps of one kind read as one run)"""
    total = 0
    for r in runs:
        n, op = int(r) >> 4, int(r) & 15
        total += n * match if op == OP_EQ else n * mismatch if op == OP_X else gap_open + (n - 1) * max(gap_open, gap_extend)
    return total


def run_tasks(queries, refs, tasks, band, **scores):
    """trace() per task (q, r, d, strand) -> (the five arrays of alignment_cases.run_tasks, [runs per task])"""
    import numpy as np
    out = [trace(queries[q], refs[r], d, band, strand, **scores) for q, r, d, strand in tasks]
    col = lambda i, dt: np.array([o[0][i] for o in out], dtype=dt)
    return (col(0, np.int32), col(1, np.uint32), col(2, np.uint32), col(3, np.uint32), col(4, np.uint32)), [o[1] for o in out]
