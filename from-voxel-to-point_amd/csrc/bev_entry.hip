// Neighbour tables of the first BEV convolution taken straight from the sparse tensor (include/fv2p_ops.h: fv2p_bev_entry_tables).
//
// HeightCompression (height_compression.py:10-26) turns the last sparse tensor [N, C] at (b, z, y, x) into the dense map
// [B, C * D, H, W], and the first block of BaseBEVBackbone (base_bev_backbone.py:27-33) runs ZeroPad2d(1) + Conv2d(C * D -> Cout, 3 x 3)
// over it.  With 3 - 10 % of the cells active that is a sparse convolution whose destination rows are all B * H * W cells: offsets
// k = z * 9 + ky * 3 + kx, the partner of (k, cell (b, oy, ox)) is the row at (b, z, oy + ky - 1, ox + kx - 1).  A row's cell is its own
// address, so the tables need no hash, no sort and no count on the host: one thread per (offset, row) writes both directions.
#include "common.hpp"

namespace fv2p {
namespace {

// t = k * n + row (rows fastest: the tab_in stores of a wave are consecutive).  tab_out was filled with -1 before.
__global__ __launch_bounds__(256) void bev_entry_tables_k(const int* __restrict__ ind, int n, int batch, int depth, int height, int width,
                                                          int* __restrict__ tab_out, int* __restrict__ tab_in) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int kvol = 9 * depth;
  if (t >= static_cast<int64_t>(kvol) * n) return;
  const int k = static_cast<int>(t / n), row = static_cast<int>(t - static_cast<int64_t>(k) * n);
  const int* p = ind + static_cast<int64_t>(row) * 4;
  const int b = p[0], z = p[1], y = p[2], x = p[3];
  const int kz = k / 9, ky = (k % 9) / 3, kx = k % 3;
  const int oy = y + 1 - ky, ox = x + 1 - kx;   // the cell whose tap (ky, kx) lies on (y, x) under padding 1, stride 1
  int cell = -1;
  // (a row outside the grid pairs with nothing: no store outside the tables whatever the coordinates hold)
  if (kz == z && b >= 0 && b < batch && y >= 0 && y < height && x >= 0 && x < width && oy >= 0 && oy < height && ox >= 0 && ox < width) {
    cell = (b * height + oy) * width + ox;
    tab_out[static_cast<int64_t>(k) * batch * height * width + cell] = row;
  }
  tab_in[t] = cell;
}

}  // namespace
}  // namespace fv2p

using namespace fv2p;

extern "C" size_t fv2p_bev_entry_tables_ws_bytes(int64_t n, int depth) { return fv2p_rulebook_pairs_ws_bytes(n, 9 * (depth > 0 ? depth : 1)); }

extern "C" int fv2p_bev_entry_tables(const int* indices, int64_t n, int batch, int depth, int height, int width, int* tab_out, int* tab_in,
                                     int* pairs, int* pair_num, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_REQUIRE(n >= 0 && batch >= 1 && depth >= 1 && height >= 1 && width >= 1, FV2P_EINVAL, "bev_entry_tables: bad sizes");
  FV2P_REQUIRE(depth <= 3, FV2P_ELIMIT, "bev_entry_tables: %d z planes give %d offsets, the conv kernels take 27", depth, 9 * depth);
  const int kvol = 9 * depth;
  const int64_t n_dst = static_cast<int64_t>(batch) * height * width;
  FV2P_REQUIRE(n_dst * kvol < (1ll << 31) && n * kvol < (1ll << 31), FV2P_ELIMIT, "bev_entry_tables: too many cells or rows");
  FV2P_REQUIRE(tab_out, FV2P_EINVAL, "bev_entry_tables: null pointer");
  FillJobs fill;
  fill.add(tab_out, sizeof(int) * static_cast<size_t>(kvol) * n_dst, 0xFFFFFFFFu);
  if (int rc = multi_fill(fill, stream)) return rc;
  if (n == 0) {
    if (pair_num) FV2P_HIP(hipMemsetAsync(pair_num, 0, sizeof(int) * kvol, stream));
    return 0;
  }
  FV2P_REQUIRE(indices && tab_in, FV2P_EINVAL, "bev_entry_tables: null pointer");
  hipLaunchKernelGGL(bev_entry_tables_k, dim3(static_cast<unsigned>(ceil_div(n * kvol, 256))), dim3(256), 0, stream, indices, static_cast<int>(n),
                     batch, depth, height, width, tab_out, tab_in);
  FV2P_LAUNCH_CHECK();
  if (pairs)   // ascending input row inside every offset (fv2p_rulebook_pairs): the weight gradient sums in one fixed order
    return fv2p_rulebook_pairs(tab_in, n, kvol, 0, pairs, pair_num, ws, ws_bytes, stream);
  return 0;
}
