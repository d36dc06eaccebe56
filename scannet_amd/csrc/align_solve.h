// align_solve.h -- the solve of one Gauss-Newton step of the global alignment, stated once for the host's loop (align.hip: align()), for the device's
// group solve (align_scan.hip: k_group_solve) and for the stand-alone program of tests/test_align_scan_cpu.py, which plain g++ compiles
// (DESIGN.md 4e "the solve" and 4h).  The matrix is the lower triangle of the symmetric N x N system, packed row by row: entry (r, c), r >= c, is
// element r (r + 1) / 2 + c; the Cholesky factor replaces it in place.  Every entry is one sum in the order align() always took it: over the pair list
// for A and b, over the column index for the factor and the two substitutions.  Only + - x / and sqrt in double; nothing here contracts.
#ifndef SCANFUSE_ALIGN_SOLVE_H
#define SCANFUSE_ALIGN_SOLVE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ALS_HD __host__ __device__
#else
#define ALS_HD
#endif
#if defined(__clang__)
#define ALS_UNROLL8 _Pragma("unroll 8")
#else
#define ALS_UNROLL8
#endif

namespace als {

constexpr double PIVOT_REL = 1e-5;     // a pivot at or below this share of its diagonal entry counts as non-positive (tk::TK_PIVOT_REL)
constexpr int GROUP_MAX = 16;          // frames of a group: 15 unknown poses, 90 unknowns
constexpr int GROUP_MAX_PAIRS = GROUP_MAX * (GROUP_MAX - 1);
constexpr int GROUP_MAX_N = 6 * (GROUP_MAX - 1);
constexpr int GROUP_THREADS = 128;     // lanes of k_group_solve's workgroup

ALS_HD inline size_t tri(int r, int c) { return (size_t)r * (size_t)(r + 1) / 2 + (size_t)c; }
// the value (u, v) of a pair's 6 x 6 block among its 21 sums (the upper triangle row by row)
ALS_HD inline int sym21(int u, int v) {
  const int a = u < v ? u : v, b = u < v ? v : u;
  return a * 6 - a * (a - 1) / 2 + (b - a);
}

// ---- assembly: what ONE pair adds to the entries with offset (u, v) inside their 6 x 6 blocks.  si / sj: the unknown slot of the pair's source /
// target frame, -1 for the fixed frame.  Pairs come in list order; different (u, v) touch different entries, so they may go to different lanes
ALS_HD inline void assemble_diag(double* A, int si, int sj, int u, int v, double h) {
  if (u < v) return;   // the lower triangle
  if (si >= 0) A[tri(6 * si + u, 6 * si + v)] += h;
  if (sj >= 0) A[tri(6 * sj + u, 6 * sj + v)] += h;
}
ALS_HD inline void assemble_off(double* A, int si, int sj, int u, int v, double h) {
  if (si < 0 || sj < 0) return;
  if (si > sj) A[tri(6 * si + u, 6 * sj + v)] -= h;
  else A[tri(6 * sj + u, 6 * si + v)] -= h;
}
ALS_HD inline void assemble_rhs(double* b, int si, int sj, int u, double g) {
  if (si >= 0) b[6 * si + u] += g;
  if (sj >= 0) b[6 * sj + u] -= g;
}

// ---- factorisation of column j, in place: the pivot, then every entry below it
ALS_HD inline double chol_pivot(const double* L, int j) {
  double s = L[tri(j, j)];
  ALS_UNROLL8
  for (int m = 0; m < j; m++) s -= L[tri(j, m)] * L[tri(j, m)];
  return s;
}
ALS_HD inline bool pivot_ok(double s, double ajj) { return s > PIVOT_REL * ajj; }
// the numerator of entry (i, j), i > j: it is divided by the root of the pivot
ALS_HD inline double chol_numerator(const double* L, int i, int j) {
  double e = L[tri(i, j)];
  ALS_UNROLL8
  for (int m = 0; m < j; m++) e -= L[tri(i, m)] * L[tri(j, m)];
  return e;
}
// L y = -b and L^T x = y, entry by entry
ALS_HD inline double forward_entry(const double* L, const double* b, const double* y, int i) {
  double e = -b[i];
  ALS_UNROLL8
  for (int m = 0; m < i; m++) e -= L[tri(i, m)] * y[m];
  return e / L[tri(i, i)];
}
ALS_HD inline double backward_entry(const double* L, const double* y, const double* x, int i, int N) {
  double e = y[i];
  ALS_UNROLL8
  for (int m = i + 1; m < N; m++) e -= L[tri(m, i)] * x[m];
  return e / L[tri(i, i)];
}

// A x = -b on one thread (the host's loop): A is replaced by its factor; false at a pivot that is not positive enough
inline bool solve_packed(double* A, const double* b, int N, double* y, double* x) {
  for (int j = 0; j < N; j++) {
    const double ajj = A[tri(j, j)], s = chol_pivot(A, j);
    if (!pivot_ok(s, ajj)) return false;
    const double ljj = sqrt(s);
    for (int i = j + 1; i < N; i++) A[tri(i, j)] = chol_numerator(A, i, j) / ljj;
    A[tri(j, j)] = ljj;
  }
  for (int i = 0; i < N; i++) y[i] = forward_entry(A, b, y, i);
  for (int i = N - 1; i >= 0; i--) x[i] = backward_entry(A, y, x, i, N);
  return true;
}

// ---- the group solve as k_group_solve maps it onto GROUP_THREADS lanes: phases that a workgroup barrier separates.  The stand-alone test
// program runs every phase for lane 0 .. GROUP_THREADS - 1 in a loop instead.

struct GroupIn {          // one group's problem
  int n;                  // members, 1..16; member 0 keeps its pose
  int npairs;             // pairs, <= 240
  uint32_t valid;         // bit k: member k takes part
  const uint16_t* pairs;  // source | target << 8, local member indices
  const double* sys;      // npairs x nsys values
  int nsys;               // 29, or 31 with the colour term's two sums
  double min_corr;        // min_pair_correspondences
};
struct GroupOut {         // one group's record, read back by the host
  double xi[GROUP_MAX * 6];     // the update of every member, 0 for a member with no unknown
  double corr, r2, ccorr, cr2;  // sums over the pairs used, in list order
  int32_t status;               // 0 solved, 1 singular, 2 fewer than two members connected to the first
  int32_t used;                 // pairs in the system
  uint32_t conn;                // bit k: member k is connected to the first
  int32_t pad;
};
struct GroupMem {         // the workgroup's LDS: 35.5 KB
  double L[GROUP_MAX_N * (GROUP_MAX_N + 1) / 2];
  double b[GROUP_MAX_N], y[GROUP_MAX_N], x[GROUP_MAX_N];
  double ljj;
  uint32_t adj[GROUP_MAX];      // bit j of adj[i]: a kept pair joins members i and j
  int8_t slot[GROUP_MAX];
  uint8_t kept[GROUP_MAX_PAIRS];
  uint32_t conn;
  int32_t N, status, bad;
};

ALS_HD inline int pair_src(uint16_t p) { return p & 255; }
ALS_HD inline int pair_dst(uint16_t p) { return p >> 8; }

// phase 1: the pairs that are kept; member t's neighbours
ALS_HD inline void phase_kept(const GroupIn& g, GroupMem& m, int t) {
  for (int p = t; p < g.npairs; p += GROUP_THREADS) {
    const int i = pair_src(g.pairs[p]), j = pair_dst(g.pairs[p]);
    m.kept[p] = ((g.valid >> i) & 1u) && ((g.valid >> j) & 1u) && g.sys[(size_t)p * g.nsys + 28] >= g.min_corr;
  }
}
ALS_HD inline void phase_adjacency(const GroupIn& g, GroupMem& m, int t) {
  if (t >= GROUP_MAX) return;
  uint32_t a = 0;
  for (int p = 0; p < g.npairs; p++) {
    if (!m.kept[p]) continue;
    const int i = pair_src(g.pairs[p]), j = pair_dst(g.pairs[p]);
    if (i == t) a |= 1u << j;
    if (j == t) a |= 1u << i;
  }
  m.adj[t] = a;
}
// phase 2 (lane 0): the members connected to the first, their slots in ascending member order, the status; then all lanes clear the system
ALS_HD inline void phase_connect(const GroupIn& g, GroupMem& m, int t) {
  if (t != 0) return;
  uint32_t reach = 1u, seen = 0u;
  while (reach != seen) {
    const uint32_t fresh = reach & ~seen;
    seen = reach;
    for (int k = 0; k < GROUP_MAX; k++)
      if ((fresh >> k) & 1u) reach |= m.adj[k];
  }
  const uint32_t conn = reach & g.valid;
  int n = 0, nconn = 0;
  for (int k = 0; k < GROUP_MAX; k++) {
    m.slot[k] = -1;
    if (k < g.n && ((conn >> k) & 1u)) {
      nconn++;
      if (k != 0) m.slot[k] = (int8_t)n++;
    }
  }
  m.conn = conn;
  m.N = 6 * n;
  m.bad = 0;
  m.status = (!(g.valid & 1u) || nconn < 2) ? 2 : 0;
}
ALS_HD inline void phase_clear(GroupMem& m, int t) {
  const int N = m.N, cells = N * (N + 1) / 2;
  for (int e = t; e < cells; e += GROUP_THREADS) m.L[e] = 0.0;
  for (int e = t; e < N; e += GROUP_THREADS) m.b[e] = 0.0;
}
// phase 3: assembly over the pair list in order.  Lanes 0..35: the diagonal blocks' (u, v), of which the 21 with u >= v work; 36..41: the right-hand side's u; 42: the sums of the
// record; 64..99: the off-diagonal blocks' (u, v)
ALS_HD inline void phase_assemble(const GroupIn& g, GroupMem& m, GroupOut& o, int t) {
  const bool diag = t < 36, rhs = t >= 36 && t < 42, sums = t == 42, off = t >= 64 && t < 100;
  if (!(diag || rhs || sums || off)) return;
  const int e = diag ? t : (off ? t - 64 : 0), u = rhs ? t - 36 : e / 6, v = e % 6;
  if (diag && u < v) return;   // the upper triangle of a diagonal block is not stored
  int used = 0;
  double corr = 0.0, r2 = 0.0, ccorr = 0.0, cr2 = 0.0;
  for (int p = 0; p < g.npairs; p++) {
    const int i = pair_src(g.pairs[p]), j = pair_dst(g.pairs[p]);
    if (!m.kept[p] || !((m.conn >> i) & 1u)) continue;
    const double* s = g.sys + (size_t)p * g.nsys;
    const int si = m.slot[i], sj = m.slot[j];
    if (diag) assemble_diag(m.L, si, sj, u, v, s[sym21(u, v)]);
    else if (off) assemble_off(m.L, si, sj, u, v, s[sym21(u, v)]);
    else if (rhs) assemble_rhs(m.b, si, sj, u, s[21 + u]);
    else {
      used++;
      r2 += s[27];
      corr += s[28];
      if (g.nsys > 29) { cr2 += s[29]; ccorr += s[30]; }
    }
  }
  if (sums) { o.used = used; o.corr = corr; o.r2 = r2; o.ccorr = ccorr; o.cr2 = cr2; }
}
// phase 4, column j: (a) lane j's pivot and its root, the lanes below hold their numerators; (b) they divide.  Lane i stands for row i and for row
// i + GROUP_THREADS (there is none: N <= 90 < GROUP_THREADS)
ALS_HD inline double phase_column_a(GroupMem& m, int j, int t) {
  if (t == j) {
    const double ajj = m.L[tri(j, j)], s = chol_pivot(m.L, j);
    if (!pivot_ok(s, ajj)) m.bad = 1;
    m.ljj = sqrt(s);
    return 0.0;
  }
  return (t > j && t < m.N) ? chol_numerator(m.L, t, j) : 0.0;
}
ALS_HD inline void phase_column_b(GroupMem& m, int j, int t, double numerator) {
  if (t > j && t < m.N) m.L[tri(t, j)] = numerator / m.ljj;
  if (t == j) m.L[tri(j, j)] = m.ljj;
}
// phase 5 (lane 0): the two substitutions
ALS_HD inline void phase_substitute(GroupMem& m, int t) {
  if (t != 0) return;
  const int N = m.N;
  for (int i = 0; i < N; i++) m.y[i] = forward_entry(m.L, m.b, m.y, i);
  for (int i = N - 1; i >= 0; i--) m.x[i] = backward_entry(m.L, m.y, m.x, i, N);
}
// phase 6: the record
ALS_HD inline void phase_record(const GroupIn& g, const GroupMem& m, GroupOut& o, int t) {
  const bool solved = m.status == 0 && !m.bad;
  if (t < GROUP_MAX * 6) {
    const int k = t / 6, s = m.slot[k];
    o.xi[t] = (solved && s >= 0) ? m.x[6 * s + t % 6] : 0.0;
  }
  if (t == 0) {
    o.status = m.status == 2 ? 2 : (m.bad ? 1 : 0);
    o.conn = m.conn;
    o.pad = 0;
    if (m.status == 2) { o.used = 0; o.corr = o.r2 = o.ccorr = o.cr2 = 0.0; }
  }
}

}  // namespace als

#endif
