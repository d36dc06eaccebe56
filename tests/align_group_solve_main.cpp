// align_group_solve_main.cpp -- the group solve of scannet_amd/csrc/align_solve.h on the CPU, run the way k_group_solve maps it: every phase for
// lane 0 .. GROUP_THREADS - 1 in a loop where the kernel has a barrier (tests/test_align_scan_cpu.py builds this with g++, once plain and once with
// -fsanitize=address,undefined, and compares its records with a Python restatement; tests/test_align_scan.py compares the kernel's with them).
//
//   align_group_solve_main <in> <out>
//   in : int32 G, nsys, min_pair_correspondences, P; int32 group_first[G + 1]; int32 pair_first[G + 1]; uint32 valid[G]; int32 local_pairs[2 P];
//        double sys[P nsys]
//   out: double xi[M 6]; int32 status[G]; int32 used[G]; uint32 conn[G]; double sums[G 4] {counts, r^2, colour counts, colour r^2}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../scannet_amd/csrc/align_solve.h"

static void solve(const als::GroupIn& g, als::GroupMem& m, als::GroupOut& o) {
  const int T = als::GROUP_THREADS;
  for (int t = 0; t < T; t++) als::phase_kept(g, m, t);
  for (int t = 0; t < T; t++) als::phase_adjacency(g, m, t);
  for (int t = 0; t < T; t++) als::phase_connect(g, m, t);
  if (m.status == 0) {
    for (int t = 0; t < T; t++) als::phase_clear(m, t);
    for (int t = 0; t < T; t++) als::phase_assemble(g, m, o, t);
    std::vector<double> numerator(T);
    for (int j = 0; j < m.N; j++) {
      for (int t = 0; t < T; t++) numerator[t] = als::phase_column_a(m, j, t);
      if (m.bad) break;
      for (int t = 0; t < T; t++) als::phase_column_b(m, j, t, numerator[t]);
    }
    if (!m.bad)
      for (int t = 0; t < T; t++) als::phase_substitute(m, t);
  }
  for (int t = 0; t < T; t++) als::phase_record(g, m, o, t);
}

template <typename V>
static bool read_all(FILE* f, std::vector<V>& v) { return v.empty() || std::fread(v.data(), sizeof(V), v.size(), f) == v.size(); }
template <typename V>
static bool write_all(FILE* f, const std::vector<V>& v) { return v.empty() || std::fwrite(v.data(), sizeof(V), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t head[4];
  if (std::fread(head, sizeof(int32_t), 4, in) != 4 || head[0] < 1 || head[3] < 0 || (head[1] != 29 && head[1] != 31)) return 2;
  const int G = head[0], nsys = head[1], P = head[3];
  std::vector<int32_t> group_first(G + 1), pair_first(G + 1), local(2 * (size_t)P);
  std::vector<uint32_t> valid(G);
  std::vector<double> sys((size_t)P * nsys);
  if (!read_all(in, group_first) || !read_all(in, pair_first) || !read_all(in, valid) || !read_all(in, local) || !read_all(in, sys)) return 2;
  std::fclose(in);
  if (group_first[0] != 0 || pair_first[0] != 0 || pair_first[G] != P) return 2;
  const int M = group_first[G];
  std::vector<double> xi((size_t)M * 6), sums((size_t)G * 4);
  std::vector<int32_t> status(G), used(G);
  std::vector<uint32_t> conn(G);
  std::vector<uint16_t> lp(P);
  for (int p = 0; p < P; p++) lp[p] = (uint16_t)(local[2 * p] | (local[2 * p + 1] << 8));
  als::GroupMem* m = new als::GroupMem;
  for (int g = 0; g < G; g++) {
    const int n = group_first[g + 1] - group_first[g], np = pair_first[g + 1] - pair_first[g];
    if (n < 1 || n > als::GROUP_MAX || np < 0 || np > als::GROUP_MAX_PAIRS) return 2;
    std::memset(m, 0, sizeof(*m));
    const als::GroupIn gi = {n, np, valid[g], lp.data() + pair_first[g], sys.data() + (size_t)pair_first[g] * nsys, nsys, (double)head[2]};
    als::GroupOut o;
    std::memset(&o, 0, sizeof(o));
    solve(gi, *m, o);
    std::memcpy(&xi[6 * (size_t)group_first[g]], o.xi, 6 * (size_t)n * sizeof(double));
    status[g] = o.status;
    used[g] = o.used;
    conn[g] = o.conn;
    sums[4 * g] = o.corr; sums[4 * g + 1] = o.r2; sums[4 * g + 2] = o.ccorr; sums[4 * g + 3] = o.cr2;
  }
  delete m;
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  const bool ok = write_all(out, xi) && write_all(out, status) && write_all(out, used) && write_all(out, conn) && write_all(out, sums);
  return (std::fclose(out) == 0 && ok) ? 0 : 2;
}
