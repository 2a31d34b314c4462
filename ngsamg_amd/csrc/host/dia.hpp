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

}  // namespace dia
