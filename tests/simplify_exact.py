"""The rules of the GPU decimation (scannet_amd/csrc/simplify_gpu.hip), stated independently of the kernels and of their checker
(oracle/simplify_rounds_oracle.c): plain Python, exact rational arithmetic (fractions.Fraction) wherever the rule is rational, mpmath at 80 digits where
a square root or an eigen-decomposition enters.  Nothing here is taken from simplify_math.h or from the checker; tests/test_simplify_stages_cpu.py
holds the checker's stages to these statements, tests/test_simplify_stages.py the kernels.

  quadrics     Q(v) = sum over the live faces at v of the plane quadric of the UN-normalised normal n = (p1 - p0) x (p2 - p0): (n n^T, -2 (n.p0) n,
               (n.p0)^2); plus, for every edge of such a face that has v as an end point and is a border edge (one live face) -- or any edge under
               planar_quadric -- the quadric of the plane through the edge perpendicular to the face, normal (n x d / |d|) * w, w = boundary_weight / 2
               on the border and a hundredth of that off it.  Every entry is rational in the coordinates: (n x d)(n x d)^T w^2 / |d|^2.
  placement    the minimiser of Q = Q(v0) + Q(v1), i.e. of x'Ax + b'x + c: A x = -b / 2 where det A > 1e-6 trace^3; otherwise the point of the solution
               set nearest the edge midpoint m, x = m + A^+ (-b/2 - A m), A^+ over the eigenvalues above 1e-9 of the largest.  Where the rank the rule
               keeps is the exact rank of A (1 or 2 by construction) A^+ is rational: A / trace^2 for rank 1, ((c2 P - A) / c1 with the range projector
               P = (c2 A - A^2) / c1, c2 = trace, c1 = the sum of the principal 2 x 2 minors, for rank 2.
  priority     max(scale * Q(x), 1e-15) / min(quality_thr, worst quality of the faces around the pair after the move), scale = 1e8 / diag^6 of the
               bounding box of all vertices, quality = 2 area / longest edge^2; no division when quality_thr is 0; 1e300 when the worst quality is 0;
               capped at 3e38.  The floor applies AFTER the scale (VCG's QuadricEpsilon, and what both the host filter and the kernel do).
  link rule    on meshes whose edges have at most two consistently oriented faces: the common neighbours of v0 and v1 are exactly the vertices
               opposite the edge, and v0 has at most 48 faces (96 ring entries, two per fan face).
  winner rule  brute force over all pairs: see check_winners.
  collapse     see collapse."""
from fractions import Fraction as Fr

import mpmath
import numpy as np

mp = mpmath.mp
mp.dps = 80

DET_RULE = Fr(1, 10 ** 6)
EIG_RULE = mpmath.mpf(10) ** -9
MAX_FAN = 48


def _pt(pos, v):
    return [Fr(float(pos[v][k])) for k in range(3)]


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _plane_quadric(n, off, w2=1):
    """(a00 a01 a02 a11 a12 a22, b0 b1 b2, c) of w2 * (n.x - off)^2"""
    return [w2 * n[0] * n[0], w2 * n[0] * n[1], w2 * n[0] * n[2], w2 * n[1] * n[1], w2 * n[1] * n[2], w2 * n[2] * n[2],
            -2 * w2 * off * n[0], -2 * w2 * off * n[1], -2 * w2 * off * n[2], w2 * off * off]


def live_faces(tri, alive=None):
    return [tuple(int(k) for k in t) for f, t in enumerate(tri) if alive is None or alive[f]]


def edge_face_counts(faces):
    cnt = {}
    for t in faces:
        for j in range(3):
            k = frozenset((t[j], t[(j + 1) % 3]))
            cnt[k] = cnt.get(k, 0) + 1
    return cnt


def neighbours(faces):
    nb = {}
    for t in faces:
        for a in t:
            nb.setdefault(a, set()).update(k for k in t if k != a)
    return nb


def quadrics(pos, tri, alive=None, boundary_weight=1.0, planar=False):
    """{vertex: ten Fractions}, by the definition above; vertices without a live face are absent (their quadric is zero)."""
    faces = live_faces(tri, alive)
    cnt = edge_face_counts(faces)
    wb = Fr(float(np.float32(boundary_weight))) / 2
    Q = {}

    def add(v, q):
        acc = Q.setdefault(v, [Fr(0)] * 10)
        Q[v] = [acc[i] + q[i] for i in range(10)]
    for t in faces:
        p = [_pt(pos, v) for v in t]
        n = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
        q = _plane_quadric(n, _dot(n, p[0]))
        for v in t:
            add(v, q)
        for j in range(3):
            a, b = t[j], t[(j + 1) % 3]
            border = cnt[frozenset((a, b))] == 1
            if not border and not planar:
                continue
            d = _sub(p[(j + 1) % 3], p[j])
            l2 = _dot(d, d)
            if l2 == 0:
                continue
            w = wb if border else wb / 100
            m = _cross(n, d)
            bq = _plane_quadric(m, _dot(m, p[j]), w * w / l2)
            add(a, bq)
            add(b, bq)
    return Q


def q_sum(Q, v0, v1):
    z = [Fr(0)] * 10
    a, b = Q.get(v0, z), Q.get(v1, z)
    return [Fr(a[i]) + Fr(b[i]) for i in range(10)]


def q_value(q, x):
    """x'Ax + b'x + c, in whatever arithmetic q and x are given"""
    return (x[0] * x[0] * q[0] + 2 * x[0] * x[1] * q[1] + 2 * x[0] * x[2] * q[2] + x[1] * x[1] * q[3] + 2 * x[1] * x[2] * q[4] + x[2] * x[2] * q[5] +
            x[0] * q[6] + x[1] * q[7] + x[2] * q[8] + q[9])


def _mat(q):
    return [[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]]


def _matvec(A, x):
    return [A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2] for i in range(3)]


def _det3(A):
    return (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
            A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))


def _mpf(x):
    return mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator) if isinstance(x, Fr) else mpmath.mpf(x)


def placement(q, p0, p1):
    """The minimiser of the quadric q (ten Fractions) for the edge p0 - p1 (three floats each) -> (x, how, unsure).  x: three Fractions or mpf;
    how: "midpoint" (A = 0), "full", "rank1", "rank2" (rational), "eigen" (mpmath); unsure: the branch cannot be told apart from its neighbour."""
    q = [Fr(v) for v in q]
    A = _mat(q)
    mid = [(Fr(float(p0[k])) + Fr(float(p1[k]))) / 2 for k in range(3)]
    r0 = [-q[6 + k] / 2 for k in range(3)]
    tr = A[0][0] + A[1][1] + A[2][2]
    if tr <= 0:
        return mid, "midpoint", False
    det = _det3(A)
    ratio = det / tr ** 3
    unsure = DET_RULE / 2 < ratio < DET_RULE * 2
    if ratio > DET_RULE:
        x = []
        for k in range(3):      # Cramer
            B = [[r0[i] if j == k else A[i][j] for j in range(3)] for i in range(3)]
            x.append(_det3(B) / det)
        return x, "full", unsure
    Am = mpmath.matrix([[_mpf(A[i][j]) for j in range(3)] for i in range(3)])
    w, U = mp.eigsy(Am)
    wmax = max(abs(v) for v in w)
    kept = [k for k in range(3) if abs(w[k]) > EIG_RULE * wmax]
    unsure = unsure or any(EIG_RULE / 10 < abs(w[k]) / wmax < EIG_RULE * 10 for k in range(3))
    r = _sub(r0, _matvec(A, mid))
    c1 = A[0][0] * A[1][1] - A[0][1] ** 2 + A[0][0] * A[2][2] - A[0][2] ** 2 + A[1][1] * A[2][2] - A[1][2] ** 2
    rank = 3 if det != 0 else (2 if c1 != 0 else 1)
    if len(kept) == rank == 1:
        step = [v / tr ** 2 for v in _matvec(A, r)]
        return [mid[k] + step[k] for k in range(3)], "rank1", unsure
    if len(kept) == rank == 2:
        A2 = [[sum(A[i][k] * A[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        P = [[(tr * A[i][j] - A2[i][j]) / c1 for j in range(3)] for i in range(3)]
        pinv = [[(tr * P[i][j] - A[i][j]) / c1 for j in range(3)] for i in range(3)]
        step = _matvec(pinv, r)
        return [mid[k] + step[k] for k in range(3)], "rank2", unsure
    x = [_mpf(v) for v in mid]
    rm = [_mpf(v) for v in r]
    for k in kept:
        proj = (U[0, k] * rm[0] + U[1, k] * rm[1] + U[2, k] * rm[2]) / w[k]
        for i in range(3):
            x[i] += U[i, k] * proj
    return x, "eigen", unsure


def scale_factor(pos):
    p = np.asarray(pos, np.float64).reshape(-1, 3)
    ext = [Fr(float(p[:, k].max())) - Fr(float(p[:, k].min())) for k in range(3)]
    d2 = _mpf(ext[0] ** 2 + ext[1] ** 2 + ext[2] ** 2)
    return mpmath.mpf(10) ** 8 / d2 ** 3 if d2 > 0 else mpmath.mpf(1)


def quality(a, b, c):
    """2 area / longest edge squared of the triangle a b c (three mpf each: sums and products of binary32 coordinates are exact at this precision);
    0 for a degenerate triangle"""
    n = _cross(_sub(b, a), _sub(c, a))
    longest = max(_dot(_sub(b, a), _sub(b, a)), _dot(_sub(c, a), _sub(c, a)), _dot(_sub(b, c), _sub(b, c)))
    if longest == 0:
        return mpmath.mpf(0)
    return mpmath.sqrt(_dot(n, n)) / longest


def priority(q, x, pos, faces, v0, v1, quality_thr, scale):
    """The priority of collapsing v0 -> v1 to the binary32 position x (evaluated there, so that placement and priority errors stay apart), as an mpf,
    the worst quality it found (None: no face around the pair besides the shared ones), and the sum of the magnitudes of the terms of Q(x) carried through
    the same scale and divisor (what a rounding error in evaluating Q(x) is relative to), and whether Q(x) CANCELS: its exact value is below 2^-29 of
    that sum, so that the binary64 evaluation (2^-53 of the sum) errs by more than binary32 resolves (2^-24) of the result.  The link rule is not part of it."""
    xf = [Fr(float(v)) for v in x]
    thr = Fr(float(np.float32(quality_thr)))
    qf = [Fr(v) for v in q]
    err = _mpf(scale) * _mpf(q_value(qf, xf))
    slack = _mpf(scale) * _mpf(q_value([abs(v) for v in qf], [abs(v) for v in xf]))
    cancels = abs(err) * 2 ** 29 < slack
    worst = None
    xm = [mpmath.mpf(float(v)) for v in x]
    for t in faces:
        for a, other in ((v0, v1), (v1, v0)):
            if a in t and other not in t:
                ql = quality(*[xm if k == a else [mpmath.mpf(float(pos[k][i])) for i in range(3)] for k in t])
                worst = ql if worst is None or ql < worst else worst
    err = max(err, mpmath.mpf(10) ** -15)
    if thr > 0:
        mq = _mpf(thr) if worst is None or worst > _mpf(thr) else worst
        err = err / mq if mq > 0 else mpmath.mpf(10) ** 300
        slack = slack / mq if mq > 0 else slack
    return min(err, mpmath.mpf(3) * mpmath.mpf(10) ** 38), worst, slack, cancels


def well_formed(faces):
    """every edge has at most two faces, and two faces on an edge run through it in opposite directions: where the link rule is stated as sets"""
    seen = {}
    for t in faces:
        if len(set(t)) != 3:
            return False
        for j in range(3):
            d = (t[j], t[(j + 1) % 3])
            if d in seen:
                return False      # the same directed edge twice: same-orientation duplicate or a third face
            seen[d] = 1
    return True


def link_accepts(faces, nb, v0, v1):
    """The link rule as sets (v0 < v1); only on well_formed meshes."""
    opposite = {k for t in faces if v0 in t and v1 in t for k in t if k != v0 and k != v1}
    fan0 = sum(1 for t in faces if v0 in t)
    return (nb[v0] & nb[v1]) == opposite and fan0 <= MAX_FAN


def _scramble(h):
    """the 32-bit finaliser of MurmurHash3 (public domain, A. Appleby), a bijection of the 32-bit words"""
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def lock_key(pri_bits, e, round_no, pass_no):
    """(priority bits, scrambled edge index salted with the round and pass): the order in which conflicting candidates yield"""
    salt = ((round_no * 3 + pass_no) * 0x9E3779B9) & 0xFFFFFFFF
    return (int(pri_bits) << 32) | _scramble(e + salt)


def check_winners(nv, tri, alive, ukey, ucnt, pri, tau, round_no, passes, taken, counters):
    """The winner rule by brute force, O(E^2).  Two edges CONFLICT when an end point of one lies in the closed ring of an end point of the other.
      * pass k's candidates: priority <= tau, no end point inside the closed rings of an earlier pass's winner;
      * a candidate wins its pass iff it holds the smallest key among the candidates of that pass that conflict with it -- so every winner does, and
        every candidate that does is a winner;
      * no two winners of the round conflict, whatever their passes; no winner of pass 2 or 3 touches a vertex marked earlier;
      * taken = the closed rings of all winners; counters = (winners, faces their edges carry, largest priority bits).
    Raises AssertionError with the offending edges."""
    faces = live_faces(tri, alive)
    nb = neighbours(faces)
    E = len(ukey)
    ends = [(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in ukey]
    closed = {v: nb.get(v, set()) | {v} for e in ends for v in e}
    reach = [closed[a] | closed[b] for a, b in ends]      # every vertex an edge's collapse reads or writes a face of
    bits = np.asarray(pri, np.float32).view(np.uint32)

    def conflict(e, w):
        return ends[w][0] in reach[e] or ends[w][1] in reach[e]
    marked = set()
    winners = []
    for k in range(3):
        cand = [e for e in range(E) if pri[e] <= tau and ends[e][0] not in marked and ends[e][1] not in marked]
        key = {e: lock_key(bits[e], e, round_no, k) for e in cand}
        assert len(set(key.values())) == len(key), "two candidates share a key"
        won = [e for e in cand if all(key[e] < key[w] for w in cand if w != e and conflict(e, w))]
        got = [e for e in range(E) if passes[e] == k + 1]
        assert got == won, "pass %d: winners %s, by the rule %s" % (k + 1, got, won)
        for e in got:
            assert ends[e][0] not in marked and ends[e][1] not in marked
        winners += got
        for e in got:
            marked |= reach[e]
    for i, e in enumerate(winners):
        for w in winners[i + 1:]:
            assert not conflict(e, w) and not conflict(w, e), "winners %d and %d conflict" % (e, w)
    assert set(np.nonzero(np.asarray(passes) > 3)[0]) == set()
    want_taken = np.zeros(nv, np.uint8)
    want_taken[sorted(marked)] = 1
    assert np.array_equal(np.asarray(taken), want_taken), "taken is not the closed rings of the winners"
    top = max([int(bits[e]) for e in winners], default=0)
    assert [int(c) for c in counters] == [len(winners), sum(int(ucnt[e]) for e in winners), top], (list(counters), len(winners))
    return winners


def collapse(pos, tri, alive, Q, ukey, edges, x):
    """The collapse of each edge named (v0 -> v1, v0 < v1), stated directly: the faces holding both vertices die; v0's other faces name v1 where they named
    v0; v1 sits at x with the sum of the two quadrics (one binary64 addition per entry); v0 is deleted; nothing else changes."""
    pos, tri, alive, Q = np.array(pos, np.float32), np.array(tri, np.uint32), np.array(alive, np.uint8), np.array(Q, np.float64)
    vdel = np.zeros(len(pos), np.uint8)
    for e in edges:
        v0, v1 = int(ukey[e]) >> 32, int(ukey[e]) & 0xFFFFFFFF
        for f in range(len(tri)):
            if not alive[f] or v0 not in tri[f]:
                continue
            if v1 in tri[f]:
                alive[f] = 0
            else:
                tri[f][tri[f] == v0] = v1
        Q[v1] = Q[v0] + Q[v1]
        pos[v1] = x[e]
        vdel[v0] = 1
    return {"pos": pos, "tri": tri, "alive": alive, "Q": Q, "vdel": vdel}
