// dia.hpp -- symmetric diagonal (DIA) image of a scalar level matrix: detection and host builder.
//
// A matrix qualifies when every entry lies on one of at most `max_diags` diagonals (col - row = const), the set of
// these offsets is symmetric, storing all of them costs at most `max_fill` x nnz, and A equals its transpose BIT FOR
// BIT.  The image then holds the upper diagonals only: offsets o_1 < ... < o_K (o_k > 0) and K row-aligned arrays
//   U_k[i] = A[i][i + o_k]   (exact 0 where the entry is absent or i + o_k >= n)
// from which the lower couplings follow as A[i][i - o_k] = U_k[i - o_k].  A Kuhn-simplex P1 matrix in natural vertex
// order has 15 diagonals (7 upper) in 3D and 7 (3 upper) in 2D, and kuhn_assemble adds (i, j) and (j, i) over the same
// simplices in the same order, so it is symmetric bit for bit.
//
// Header-only: the host library exposes it as amgh_dia_detect / amgh_dia_image, the device library runs it at
// amgx_create.  `par(nblocks, f)` runs f(block) for block = 0 .. nblocks - 1, in any order and possibly concurrently.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace dia {

constexpr int MAX_DIAGS = 16;          // distinct offsets, diagonal included
constexpr int MAX_UPPER = MAX_DIAGS / 2;
constexpr int64_t ROW_BLOCK = 1 << 14;

// refusal codes of detect()
enum { NOT_SQUARE = -1, TOO_MANY_DIAGS = -2, NOT_SYMMETRIC_PATTERN = -3, TOO_MUCH_FILL = -4, NOT_BITWISE_SYMMETRIC = -5, NO_COUPLINGS = -6 };

// returns K > 0 (offsets_out[0 .. K) = the upper offsets, ascending) or a refusal code
template <class Par>
int detect(int64_t n_rows, int64_t n_cols, const int64_t* rowptr, const int32_t* col, const double* val, int max_diags, double max_fill,
           int32_t* offsets_out, Par&& par) {
  if (n_rows <= 0 || n_rows != n_cols || n_rows > (int64_t)2147483647) return NOT_SQUARE;
  max_diags = std::max(1, std::min(max_diags, MAX_DIAGS));
  const int64_t nb = (n_rows + ROW_BLOCK - 1) / ROW_BLOCK;
  // 1. the distinct offsets, per row block (a block stops collecting once it has more than max_diags)
  std::vector<std::vector<int64_t>> offs((size_t)nb);
  par(nb, [&](int64_t blk) {
    std::vector<int64_t>& o = offs[(size_t)blk];
    const int64_t i1 = std::min(n_rows, (blk + 1) * ROW_BLOCK);
    for (int64_t i = blk * ROW_BLOCK; i < i1 && (int)o.size() <= max_diags; ++i)
      for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int64_t d = (int64_t)col[k] - i;
        auto it = std::lower_bound(o.begin(), o.end(), d);
        if (it == o.end() || *it != d) {
          o.insert(it, d);
          if ((int)o.size() > max_diags) break;
        }
      }
  });
  std::vector<int64_t> all;
  for (const auto& o : offs) {
    for (int64_t d : o) {
      auto it = std::lower_bound(all.begin(), all.end(), d);
      if (it == all.end() || *it != d) all.insert(it, d);
    }
    if ((int)all.size() > max_diags) return TOO_MANY_DIAGS;
  }
  // 2. symmetric offset set
  for (size_t a = 0; a < all.size(); ++a)
    if (all[a] != -all[all.size() - 1 - a]) return NOT_SYMMETRIC_PATTERN;
  int K = 0;
  for (int64_t d : all) if (d > 0) offsets_out[K++] = (int32_t)d;
  if (K == 0) return NO_COUPLINGS;
  // 3. zero fill of the image: every stored diagonal spans n rows
  const int64_t nnz = rowptr[n_rows];
  if ((double)all.size() * (double)n_rows > max_fill * (double)nnz) return TOO_MUCH_FILL;
  // 4. A[i][j] and A[j][i] are the same bits (every entry has its mirror)
  std::vector<char> bad((size_t)nb, 0);
  par(nb, [&](int64_t blk) {
    const int64_t i1 = std::min(n_rows, (blk + 1) * ROW_BLOCK);
    for (int64_t i = blk * ROW_BLOCK; i < i1; ++i)
      for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int64_t j = col[k];
        if (j == i) continue;
        const int32_t* b = col + rowptr[j];
        const int32_t* e = col + rowptr[j + 1];
        const int32_t* p = std::lower_bound(b, e, (int32_t)i);
        if (p == e || *p != (int32_t)i || std::memcmp(&val[k], &val[rowptr[j] + (p - b)], sizeof(double)) != 0) { bad[(size_t)blk] = 1; return; }
      }
  });
  for (char c : bad) if (c) return NOT_BITWISE_SYMMETRIC;
  return K;
}

// the K upper arrays (out: K * n_rows doubles, U_k at out + k * n_rows) of a matrix detect() accepted with these offsets
template <class Par>
void upper_image(int64_t n_rows, const int64_t* rowptr, const int32_t* col, const double* val, int K, const int32_t* offsets, double* out,
                 Par&& par) {
  const int64_t nb = (n_rows + ROW_BLOCK - 1) / ROW_BLOCK;
  par(nb, [&](int64_t blk) {
    const int64_t i0 = blk * ROW_BLOCK, i1 = std::min(n_rows, (blk + 1) * ROW_BLOCK);
    for (int q = 0; q < K; ++q) std::fill(out + q * n_rows + i0, out + q * n_rows + i1, 0.0);
    for (int64_t i = i0; i < i1; ++i)
      for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int64_t d = (int64_t)col[k] - i;
        if (d <= 0) continue;
        for (int q = 0; q < K; ++q)
          if (offsets[q] == d) { out[q * n_rows + i] = val[k]; break; }
      }
  });
}

// ---------------------------------------------------------------------------------------------------
// Lexicographic grids and box chunks (dia_box_pre_restrict_kernel).
//
// The K upper offsets of a level whose rows are the vertices of an nx x ny x nz grid in lexicographic order (x fastest) are
// sums o_k = dx + dy * sy + dz * sz with dx, dy, dz in {0, 1}, sy = nx and sz = nx * ny.  grid_of() recognises that from the
// offsets alone; box_grid() then cuts the grid into boxes of whole grid lines, nx x yc x zc rows (clipped at the grid's edge,
// never padded), numbered y fastest, then z.  A box is the chunk of one workgroup: most neighbours of a row are rows of the same
// box, whose x_j = omega * (dinv_j * b_j) the workgroup hands over through LDS instead of reading b_j and dinv_j again.
// Inside a box the rows are numbered line by line (y fastest, then z): local = (lz * lines_y + ly) * nx + x.
// The geometry helpers are shared with the kernel (DIA_HD), so that the CPU tests check the very arithmetic the device runs.
#ifdef __HIPCC__
#define DIA_HD __host__ __device__ inline
#else
#define DIA_HD inline
#endif

constexpr int BOX_MAX_LINES = 8;       // grid lines per box
constexpr int BOX_MAX_ROWS = 2048;     // rows per box (512 lanes x 4 rows; the local index of the restriction data is 16-bit)
constexpr int BOX_MIN_ROWS = 48;       // a full box must fill 3/4 of one wave at least

struct Grid {
  int64_t nx = 0, ny = 0, nz = 0;      // nz = 1: a 2D grid
  int dx[MAX_UPPER] = {}, dy[MAX_UPPER] = {}, dz[MAX_UPPER] = {};
};

// true (and g filled) when offsets[0 .. K) are those of a lexicographic grid of n rows; false: not a grid (fewer than two
// offsets, an offset that does not decompose, n not divisible)
inline bool grid_of(int64_t n, int K, const int32_t* off, Grid& g) {
  if (K < 2 || K > MAX_UPPER || off[0] != 1 || off[1] < 2) return false;
  const int64_t sy = off[1];
  int64_t sz = 0;
  for (int k = 2; k < K; ++k) if (off[k] > sy + 1) { sz = off[k]; break; }
  if (sz ? (sz % sy != 0 || n % sz != 0) : n % sy != 0) return false;
  g = Grid();
  g.nx = sy;
  g.ny = sz ? sz / sy : n / sy;
  g.nz = sz ? n / sz : 1;
  for (int k = 0; k < K; ++k) {
    bool found = false;
    for (int c = 1; c < (sz ? 8 : 4) && !found; ++c)
      if ((c & 1) + ((c >> 1) & 1) * sy + ((c >> 2) & 1) * sz == off[k]) { g.dx[k] = c & 1; g.dy[k] = (c >> 1) & 1; g.dz[k] = (c >> 2) & 1; found = true; }
    if (!found) return false;
  }
  return true;
}

// the boxes of a grid, as the kernel takes them (plain data)
struct BoxGrid {
  int nx, ny, nz;                      // the grid
  int yc, zc;                          // a full box: nx x yc x zc rows
  int nby, nbz;                        // boxes in y and z
  int dmask;                           // bits 3k, 3k + 1, 3k + 2: dx, dy, dz of diagonal k
  DIA_HD int n_boxes() const { return nby * nbz; }
  DIA_HD int box_rows() const { return nx * yc * zc; }
};

// yc x zc lines per box (0 x 0: 2 x 4 in 3D, 8 x 1 in 2D), halved -- z first -- until a box has at most BOX_MAX_ROWS rows.
// false: the grid takes no boxes (a line longer than a box may be, a full box below BOX_MIN_ROWS rows, a shape of more than
// BOX_MAX_LINES lines, more rows than 32-bit indices hold)
inline bool box_grid(const Grid& g, int K, int yc, int zc, BoxGrid& b) {
  if (yc <= 0 || zc <= 0) { yc = g.nz > 1 ? 2 : 8; zc = g.nz > 1 ? 4 : 1; }
  if (g.nz == 1) zc = 1;
  if (yc * zc > BOX_MAX_LINES || g.nx > BOX_MAX_ROWS || g.nx * g.ny * g.nz > (int64_t)2147483647) return false;
  while (g.nx * yc * zc > BOX_MAX_ROWS) { if (zc > 1) zc = (zc + 1) / 2; else yc = (yc + 1) / 2; }
  if (g.nx * yc * zc < BOX_MIN_ROWS) return false;
  b.nx = (int)g.nx; b.ny = (int)g.ny; b.nz = (int)g.nz;
  b.yc = yc; b.zc = zc;
  b.nby = (int)((g.ny + yc - 1) / yc); b.nbz = (int)((g.nz + zc - 1) / zc);
  b.dmask = 0;
  for (int k = 0; k < K; ++k) b.dmask |= (g.dx[k] | g.dy[k] << 1 | g.dz[k] << 2) << (3 * k);
  return true;
}

// one box: its first line and its (clipped) numbers of lines
struct BoxAt { int y0, z0, ly, lz; };
DIA_HD BoxAt box_at(const BoxGrid& g, int box) {
  BoxAt a;
  const int bz = box / g.nby, by = box - bz * g.nby;
  a.y0 = by * g.yc; a.z0 = bz * g.zc;
  a.ly = g.ny - a.y0 < g.yc ? g.ny - a.y0 : g.yc;
  a.lz = g.nz - a.z0 < g.zc ? g.nz - a.z0 : g.zc;
  return a;
}
DIA_HD int box_nrows(const BoxGrid& g, const BoxAt& a) { return g.nx * a.ly * a.lz; }

// a row of the box by its local index: x and line (y, z) inside the box
struct BoxRow { int x, y, z; };
DIA_HD BoxRow box_row(const BoxGrid& g, const BoxAt& a, int local) {
  int line = 0, z = 0;
  for (int q = 1; q < BOX_MAX_LINES; ++q) line += local >= q * g.nx;         // (local < lines * nx bounds both sums)
  for (int q = 1; q < BOX_MAX_LINES; ++q) z += line >= q * a.ly;
  return BoxRow{local - line * g.nx, line - z * a.ly, z};
}
DIA_HD int box_global(const BoxGrid& g, const BoxAt& a, const BoxRow& r) { return ((a.z0 + r.z) * g.ny + (a.y0 + r.y)) * g.nx + r.x; }

// is row -/+ o_k (up = false / true) a row of the same box?  Its local index is then local -/+ box_local_offset(g, a, k).
// (row + o_k with x + dx = nx is the first vertex of the next line -- a structural zero of U_k, but the same rule holds.)
DIA_HD bool box_has(const BoxGrid& g, const BoxAt& a, const BoxRow& r, int k, bool up) {
  const int dx = (g.dmask >> (3 * k)) & 1, dy = (g.dmask >> (3 * k + 1)) & 1, dz = (g.dmask >> (3 * k + 2)) & 1;
  if (up) return r.y + dy + (r.x + dx >= g.nx ? 1 : 0) < a.ly && r.z + dz < a.lz;
  return r.y - dy - (r.x - dx < 0 ? 1 : 0) >= 0 && r.z - dz >= 0;
}
DIA_HD int box_local_offset(const BoxGrid& g, const BoxAt& a, int k) {
  const int dx = (g.dmask >> (3 * k)) & 1, dy = (g.dmask >> (3 * k + 1)) & 1, dz = (g.dmask >> (3 * k + 2)) & 1;
  return dx + (dy + dz * a.ly) * g.nx;
}

// the rows of every box as runs (first row, length): the lines of box c are runs run_ptr[c] .. run_ptr[c + 1), in the order of
// the local index
struct BoxRuns {
  std::vector<int64_t> first;
  std::vector<int32_t> len;
  std::vector<int64_t> run_ptr;
  int64_t n_boxes() const { return (int64_t)run_ptr.size() - 1; }
};
inline BoxRuns box_runs(const BoxGrid& g) {
  BoxRuns R;
  R.run_ptr.push_back(0);
  for (int c = 0; c < g.n_boxes(); ++c) {
    const BoxAt a = box_at(g, c);
    for (int z = 0; z < a.lz; ++z)
      for (int y = 0; y < a.ly; ++y) {
        R.first.push_back(box_global(g, a, BoxRow{0, y, z}));
        R.len.push_back(g.nx);
      }
    R.run_ptr.push_back((int64_t)R.first.size());
  }
  return R;
}

}  // namespace dia
