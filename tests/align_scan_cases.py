"""What the tests of the scan alignment share (tests/test_align_scan_cpu.py without a GPU, tests/test_align_scan.py on one): the plan rule and the group
solve restated in Python from DESIGN.md 4e / 4h, the hierarchy on the CPU checker (al_pairs / al_align / al_spread of tests/align_checker.c), the
stand-alone program of tests/align_group_solve_main.cpp and the problems it and the kernel are given.  Scenes come from tests/solver_scenes.py."""
import ctypes as C
import functools
import math
import os
import shutil
import subprocess

import numpy as np

from tests import solver_scenes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240
MAX_PAIRS = 4096


def finite(poses):
    return np.isfinite(np.asarray(poses, np.float32).reshape(-1, 16)[:, :12]).all(axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The plan, DESIGN.md 4h
# ---------------------------------------------------------------------------------------------------------------------------------------------
def python_plan(poses, a, group_size, top_frames, count_pairs):
    """-> (groups [(level, [frames])], top [frames], levels).  count_pairs(poses [n,16]) is the pair rule's count."""
    poses = np.asarray(poses, np.float32).reshape(-1, 16)
    L = [int(k) for k in np.flatnonzero(finite(poses))]
    groups, level = [], 0
    while len(L) > top_frames or count_pairs(poses[L]) > MAX_PAIRS:
        runs = [L[at:at + group_size] for at in range(0, len(L), group_size)]
        groups += [(level, r) for r in runs]
        L = [r[0] for r in runs]
        level += 1
    return groups, L, level


def checker_pairs(poses, a):
    """al_pairs of tests/align_checker.c -> int32 [P,2]."""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    cap = max(1, len(poses) * (len(poses) - 1))
    out = np.zeros((cap, 2), np.int32)
    n = C.c_uint64(0)
    assert ss.align_lib().al_pairs(ss.ptr(poses), len(poses), C.byref(a), ss.ptr(out), cap, C.byref(n)) == 0
    assert n.value <= cap
    return out[:n.value].copy()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The hierarchy on the CPU checker
# ---------------------------------------------------------------------------------------------------------------------------------------------
def checker_spread(poses, new_first):
    """al_spread(poses, keyframes {0}, {new_first})."""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    keys = np.zeros(1, np.uint64)
    new = np.ascontiguousarray(new_first, np.float32).reshape(1, 16)
    out = np.empty_like(poses)
    assert ss.align_lib().al_spread(ss.ptr(poses), len(poses), ss.ptr(keys), 1, ss.ptr(new), ss.ptr(out)) == 0
    return out


def chain(depth, poses, a, group_size, top_frames, solve, pairs_of, spread):
    """The scan call composed from single solves: solve(depth [n], poses [n,16], pairs) -> (poses [n,16], result); pairs_of(poses) -> [P,2];
    spread(poses [n,16], new first pose) -> [n,16].  -> (poses [K,16], [(level, frames, result)], top frames, top result)."""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    groups, top, levels = python_plan(poses, a, group_size, top_frames, lambda p: len(pairs_of(p)))
    out = poses.copy()
    solved = []
    for level, frames in groups:
        if len(frames) < 2:
            solved.append((level, frames, poses[frames].copy(), None))
            continue
        got, res = solve(depth[frames], poses[frames], pairs_of(poses[frames]))
        solved.append((level, frames, got, res))
    top_res = None
    if len(top) >= 2:
        got, top_res = solve(depth[top], poses[top], pairs_of(poses[top]))
        out[top] = got
    for lv in range(levels - 1, -1, -1):
        for level, frames, got, res in solved:
            if level == lv:
                out[frames[1:]] = spread(got, out[frames[0]])[1:]
    return out, [(lv, fr, res) for lv, fr, _, res in solved], top, top_res


def checker_chain(depth, poses, a, group_size, top_frames, fr=None):
    fr = fr or ss.align_frame(W, H)

    def solve(d, p, pairs):
        rc, out, res = ss.cpu_align(d, p, pairs, a, fr)
        assert rc == 0
        return out, res

    return chain(depth, poses, a, group_size, top_frames, solve, lambda p: checker_pairs(p, a), checker_spread)


# the four shapes of the issue's table: name -> (views, group_size, top_frames, the lost frame or None)
SHAPES = {"12_by_4_under_3": (12, 4, 3, None), "12_by_2_by_2_under_3": (12, 2, 3, None), "12_frame_5_lost": (12, 4, 3, 5), "13_by_4_under_4": (13, 4, 4, None)}


@functools.lru_cache(maxsize=None)
def arc(n):
    return ss.corner_arc(n, W, H, metres=0.1)


def shape_input(name):
    """-> (depth [n, H*W], truth [n,4,4], start [n,16], group_size, top_frames)."""
    n, g, t, lost = SHAPES[name]
    depth, truth, start = arc(n)
    start = start.reshape(n, 16).copy()
    if lost is not None:
        start[lost] = -np.inf
    return depth, truth, start, g, t


@functools.lru_cache(maxsize=None)
def shape_chain(name):
    """The CPU chain's answer on a shape (computed once, shared by the CPU and the GPU tests)."""
    from scannet_amd import fusion
    depth, truth, start, g, t = shape_input(name)
    return checker_chain(depth, start, fusion.default_align_params(), g, t)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# One group's solve in Python floats (IEEE double, one rounding per operation), DESIGN.md 4e: the pairs kept, the frames connected to the first,
# the slots, A and b over the pair list, Cholesky and the two substitutions with every sum in index order
# ---------------------------------------------------------------------------------------------------------------------------------------------
def python_group_solve(n, pairs, valid, sys, min_corr):
    """-> (xi [n][6], status, used, conn bits, (counts, r2, colour counts, colour r2))."""
    P = len(pairs)
    kept = [bool(valid[i] and valid[j] and sys[p][28] >= min_corr) for p, (i, j) in enumerate(pairs)]
    parent = list(range(n))

    def root(k):
        while parent[k] != k:
            k = parent[k]
        return k

    for p, (i, j) in enumerate(pairs):
        if kept[p]:
            ra, rb = root(i), root(j)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    conn = [bool(valid[k]) and root(k) == root(0) for k in range(n)]
    bits = sum(1 << k for k in range(n) if conn[k])
    zero = [[0.0] * 6 for _ in range(n)]
    if not valid[0] or sum(conn) < 2:
        return zero, 2, 0, bits, (0.0, 0.0, 0.0, 0.0)
    slot, m = [-1] * n, 0
    for k in range(1, n):
        if conn[k]:
            slot[k] = m
            m += 1
    N = 6 * m
    A = [[0.0] * N for _ in range(N)]
    b = [0.0] * N
    used, corr, r2, ccorr, cr2 = 0, 0.0, 0.0, 0.0, 0.0
    for p, (i, j) in enumerate(pairs):
        if not kept[p] or not conn[i]:
            continue
        s = [float(x) for x in sys[p]]
        Hm = [[0.0] * 6 for _ in range(6)]
        k = 0
        for u in range(6):
            for v in range(u, 6):
                Hm[u][v] = Hm[v][u] = s[k]
                k += 1
        si, sj = slot[i], slot[j]
        for u in range(6):
            for v in range(6):
                if si >= 0:
                    A[6 * si + u][6 * si + v] += Hm[u][v]
                if sj >= 0:
                    A[6 * sj + u][6 * sj + v] += Hm[u][v]
                if si >= 0 and sj >= 0:
                    A[6 * si + u][6 * sj + v] -= Hm[u][v]
                    A[6 * sj + u][6 * si + v] -= Hm[u][v]
            if si >= 0:
                b[6 * si + u] += s[21 + u]
            if sj >= 0:
                b[6 * sj + u] -= s[21 + u]
        used += 1
        r2 += s[27]
        corr += s[28]
        if len(s) > 29:
            cr2 += s[29]
            ccorr += s[30]
    sums = (corr, r2, ccorr, cr2)
    Lm = [[0.0] * N for _ in range(N)]
    for j in range(N):
        s = A[j][j]
        for q in range(j):
            s -= Lm[j][q] * Lm[j][q]
        if not s > 1e-5 * A[j][j]:
            return zero, 1, used, bits, sums
        Lm[j][j] = math.sqrt(s)
        for i in range(j + 1, N):
            e = A[i][j]
            for q in range(j):
                e -= Lm[i][q] * Lm[j][q]
            Lm[i][j] = e / Lm[j][j]
    y, x = [0.0] * N, [0.0] * N
    for i in range(N):
        e = -b[i]
        for q in range(i):
            e -= Lm[i][q] * y[q]
        y[i] = e / Lm[i][i]
    for i in range(N - 1, -1, -1):
        e = y[i]
        for q in range(i + 1, N):
            e -= Lm[q][i] * x[q]
        x[i] = e / Lm[i][i]
    xi = [[x[6 * slot[k] + c] if slot[k] >= 0 else 0.0 for c in range(6)] for k in range(n)]
    return xi, 0, used, bits, sums


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The problems of the stage tests: (name, n, pairs [P,2], valid [n], sys [P,31])
# ---------------------------------------------------------------------------------------------------------------------------------------------
def synthetic_group(n, seed, lo=-6, hi=6):
    """A chain of n frames with both directions of every neighbour pair and of every second neighbour; each pair's 6 x 6 block is J^T J of 40 random
    rows scaled by D = diag(10^e), e spread over lo/2 .. hi/2, so that the diagonal spans 10^lo .. 10^hi."""
    rng = np.random.default_rng(seed)
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j and abs(i - j) <= 2]
    scale = 10.0 ** np.linspace(lo / 2.0, hi / 2.0, 6)
    sys = np.zeros((len(pairs), 31))
    for p in range(len(pairs)):
        J = rng.standard_normal((40, 6)) * scale
        r = rng.standard_normal(40) * 1e-2
        Hm, g = J.T @ J, J.T @ r
        sys[p, :21] = [Hm[u][v] for u in range(6) for v in range(u, 6)]
        sys[p, 21:27] = g
        sys[p, 27] = float(r @ r)
        sys[p, 28] = 1000.0 + p
    return np.array(pairs, np.int32), sys


@functools.lru_cache(maxsize=None)
def stage_problems():
    from scannet_amd import fusion
    a = fusion.default_align_params()
    fr = ss.align_frame(W, H)
    depth, truth, start = arc(16)
    start = start.reshape(16, 16)
    out = []
    for n in (2, 4, 16):
        pairs = checker_pairs(start[:n], a)
        rc, sys = ss.cpu_align_system(depth[:n], start[:n], pairs, a, fr)
        assert rc == 0
        out.append(("arc%d" % n, n, pairs, [1] * n, sys))
    cases = ss.structure_cases(arc(6), W, H)
    for name in ("thin", "planes"):
        d, poses, pairs = cases[name]
        rc, sys = ss.cpu_align_system(d, poses, pairs, a, fr)
        assert rc == 0
        if name == "thin":   # its frame 1 goes too, so that no frame is connected to the first: status 2
            sys = sys.copy()
            sys[:, 28] = np.minimum(sys[:, 28], 100.0)
        out.append((name, len(poses), pairs, [1] * len(poses), sys))
    d, poses, pairs = cases["thin"]
    rc, sys = ss.cpu_align_system(d, poses, pairs, a, fr)
    out.append(("thin_one_left", 3, pairs, [1, 1, 1], sys))   # frame 2 unconnected, frame 1 solved
    pairs, sys = synthetic_group(5, 7)
    out.append(("spd_1e-6_1e6", 5, pairs, [1] * 5, sys))
    out.append(("spd_member_2_invalid", 5, pairs, [1, 1, 0, 1, 1], sys))
    pairs, sys = synthetic_group(16, 11, -3, 3)
    out.append(("spd_16", 16, pairs, [1] * 16, sys))
    return out, int(a.min_pair_correspondences)


def python_records(problems, min_corr):
    return [python_group_solve(n, [tuple(int(x) for x in p) for p in pairs], valid, sys, float(min_corr)) for _, n, pairs, valid, sys in problems]


def stage_arrays(problems):
    """-> (group_first, pair_first, valid masks, local pairs [P,2], sys [P,31])."""
    gf, pf = [0], [0]
    for _, n, pairs, valid, sys in problems:
        gf.append(gf[-1] + n)
        pf.append(pf[-1] + len(pairs))
    masks = np.array([sum(1 << k for k, v in enumerate(valid) if v) for _, _, _, valid, _ in problems], np.uint32)
    return (np.array(gf, np.int32), np.array(pf, np.int32), masks, np.ascontiguousarray(np.concatenate([p for _, _, p, _, _ in problems]), np.int32),
            np.ascontiguousarray(np.concatenate([s for _, _, _, _, s in problems]), np.float64))


def records_bytes(xi, status, used, conn, sums):
    """One byte string per record set, for bit-for-bit comparison."""
    return (np.ascontiguousarray(xi, np.float64).tobytes(), np.ascontiguousarray(status, np.int32).tobytes(), np.ascontiguousarray(used, np.int32).tobytes(),
            np.ascontiguousarray(conn, np.uint32).tobytes(), np.ascontiguousarray(sums, np.float64).tobytes())


def python_records_arrays(problems, min_corr):
    recs = python_records(problems, min_corr)
    xi = np.array([row for r in recs for row in r[0]], np.float64)
    return xi, [r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs], np.array([r[4] for r in recs], np.float64)


def build_program(directory, sanitize):
    """tests/align_group_solve_main.cpp compiled by g++ -> the program's path."""
    exe = os.path.join(str(directory), "align_group_solve" + ("_san" if sanitize else ""))
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "align_group_solve_main.cpp")]
    if sanitize:
        cmd[1:1] = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd, check=True)
    return exe


def run_program(exe, directory, problems, min_corr, tag=""):
    """-> (xi [M,6], status [G], used [G], conn [G], sums [G,4]) as the program wrote them."""
    gf, pf, masks, local, sys = stage_arrays(problems)
    G, P, M = len(problems), len(local), int(gf[-1])
    fin, fout = os.path.join(str(directory), "in%s.bin" % tag), os.path.join(str(directory), "out%s.bin" % tag)
    with open(fin, "wb") as f:
        f.write(np.array([G, sys.shape[1], min_corr, P], np.int32).tobytes() + gf.tobytes() + pf.tobytes() + masks.tobytes() + local.tobytes() + sys.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(fout, "rb").read()
    assert len(raw) == M * 48 + G * 12 + G * 32
    xi = np.frombuffer(raw, np.float64, M * 6).reshape(M, 6)
    o = M * 48
    status, used, conn = np.frombuffer(raw, np.int32, G, o), np.frombuffer(raw, np.int32, G, o + 4 * G), np.frombuffer(raw, np.uint32, G, o + 8 * G)
    return xi, status, used, conn, np.frombuffer(raw, np.float64, 4 * G, o + 12 * G).reshape(G, 4)


def have_gxx():
    return shutil.which("g++") is not None
