// merit.hip -- (MSE, SSIM, PSNR) of a whole batch of image pairs in float64 (the reference's compare, ctvae/helper_functions.py:394-418,
// with scikit-image 0.18's structural_similarity and peak_signal_noise_ratio): ref, test [n][X][Y], both float32 or both float64, ->
// out [n][3] float64.  Three launches whatever n, X, Y are.  float32 pixels are widened to double first; every operation below is one
// float64 operation (-ffp-contract=off: no fused multiply-add), so a float64 restatement in the same order gives the same bits
// (tests/np_twin_merit.py; only the log10 of the PSNR is a library function).
//
// Per pair, with r = ref[k], t = test[k]:
//   mse  = (sum (r - t)^2) / (X Y)
//   R    = max r - min r                              (a NaN pixel of r makes R NaN, as numpy's max does)
//   win  = 7 if min(X, Y) >= 7, else the largest odd number <= min(X, Y);  NP = win^2;  cov_norm = NP / (NP - 1)
//   at every window position (i, j), i < Xo = X - win + 1, j < Yo = Y - win + 1 (the window r[i .. i + win)[j .. j + win)):
//     W(q) = the window's sum of q, rows ascending, each row's sum its columns ascending:
//            W(q) = ((row_i + row_(i+1)) + ...) + row_(i+win-1),  row_a = ((q[a][j] + q[a][j+1]) + ...) + q[a][j+win-1]
//     ux = W(r) / NP, uy = W(t) / NP, uxx = W(r r) / NP, uyy = W(t t) / NP, uxy = W(r t) / NP
//     vx = cov_norm (uxx - ux ux), vy = cov_norm (uyy - uy uy), vxy = cov_norm (uxy - ux uy)
//     a1 = 0.01 R, c1 = a1 a1, a2 = 0.03 R, c2 = a2 a2
//     S = (((2 ux) uy + c1) ((2 vxy) + c2)) / (((ux ux + uy uy) + c1) ((vx + vy) + c2))
//   ssim = (sum S) / (Xo Yo)
//   psnr = +inf if mse == 0 (scikit-image's rule), else 10 log10((R R) / mse)
//
// Launch 1, merit_range_kernel: the flat image is cut into chunks of kMeritChunk = 4096 pixels, one workgroup of 256 threads each
// (block = pair * chunks + chunk).  It leaves the chunk's sum of (r - t)^2, min r and max r in the workspace: R must be known before any S.
// Launch 2, merit_ssim_kernel: the Xo x Yo window positions are cut into tiles of kMeritTile x kMeritTile = 32 x 32 (tile = tile row *
// tiles per row + tile column; block = pair * tiles + tile).  A workgroup first takes min r, max r over the pair's chunks (min and max
// are exact: any order, same value), then loads its (32 + win - 1)^2 pixels of r and t into LDS as doubles (0 outside the image: only
// positions outside Xo x Yo read those), forms the row sums of the five quantities in LDS, then the window sums and S of its positions
// in registers, and leaves the tile's sum of S in the workspace.  No S is written to memory.
// Launch 3, merit_finish_kernel: one workgroup of 64 threads per pair adds the chunks' and the tiles' partial sums and writes the
// three numbers.
//
// The order of every sum -- one rule, ST(v, w) for a list v and a width w (no floating-point atomics anywhere):
//   thread u < w:   P_u = ((0 + v[u]) + v[u + w]) + v[u + 2 w] + ...          its elements ascending (elements that do not exist: skipped)
//   then log2(w) halving steps through LDS:  for h = w / 2, w / 4, ..., 1:  P_u = P_u + P_(u + h) for u < h;   ST = P_0
//   chunk c:   Q_c   = ST(the chunk's (r - t)^2 in flat pixel order, 256)
//   tile  b:   S_b   = ST(the tile's S in row-major order of its 32 x 32 positions, with positions outside Xo x Yo left out, 256)
//   pair:      sum (r - t)^2 = ST(Q_0, Q_1, ..., 64);   sum S = ST(S_0, S_1, ..., 64)       chunks and tiles ascending
// Nothing depends on n or on the pair's index k, and the same call gives the same bits on every run.
//
// Workspace: per pair 3 * chunks + tiles doubles, chunks = ceil(X Y / 4096) <= tiles: at most 4 * tiles * n doubles.
// LDS of launch 2: 2 * 38 * 38 + 5 * 38 * 32 + 2 * 256 doubles = 75840 bytes (dynamic; two workgroups per CU).
#include <climits>
#include <cmath>

#include "common.h"

namespace ctpvae {

constexpr int kMeritThreads = 256;
constexpr int kMeritChunk = 4096;                 // pixels of a launch-1 workgroup
constexpr int kMeritTile = 32;                    // window positions per tile edge
constexpr int kMeritMaxWin = 7;
constexpr int kMeritHalo = kMeritTile + kMeritMaxWin - 1;     // 38: edge of a tile's pixel block
constexpr int kMeritFinishThreads = 64;
constexpr int kMeritPxDoubles = 2 * kMeritHalo * kMeritHalo;              // r, t
constexpr int kMeritRowDoubles = 5 * kMeritHalo * kMeritTile;             // row sums of r, t, rr, tt, rt
constexpr int kMeritSsimLdsBytes = (kMeritPxDoubles + kMeritRowDoubles + 2 * kMeritThreads) * (int)sizeof(double);

struct MeritShape {
    int n, X, Y, win, Xo, Yo, tiles_c, tiles, chunks;
    long long pix;      // X * Y
};

inline int merit_win(int X, int Y)
{
    const int m = X < Y ? X : Y;
    return m >= kMeritMaxWin ? kMeritMaxWin : (m % 2 ? m : m - 1);
}

inline MeritShape merit_shape(int n, int X, int Y)
{
    MeritShape sh;
    sh.n = n, sh.X = X, sh.Y = Y, sh.win = merit_win(X, Y);
    sh.Xo = X - sh.win + 1, sh.Yo = Y - sh.win + 1;
    sh.tiles_c = ceil_div(sh.Yo, kMeritTile);
    sh.tiles = ceil_div(sh.Xo, kMeritTile) * sh.tiles_c;
    sh.pix = (long long)X * Y;
    sh.chunks = (int)((sh.pix + kMeritChunk - 1) / kMeritChunk);
    return sh;
}

// NaN-propagating min / max (numpy's): a NaN on either side stays
__device__ __forceinline__ double merit_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double merit_max(double a, double b) { return (b > a || b != b) ? b : a; }

// the halving steps of ST over red[0 .. W); every thread of the workgroup calls it; the result is red[0]
template <int W> __device__ __forceinline__ void merit_halve_sum(double *red, int u)
{
    __syncthreads();
#pragma unroll
    for (int h = W / 2; h >= 1; h >>= 1) {
        if (u < h) red[u] = red[u] + red[u + h];
        __syncthreads();
    }
}

template <int W> __device__ __forceinline__ void merit_halve_range(double *lo, double *hi, int u)
{
    __syncthreads();
#pragma unroll
    for (int h = W / 2; h >= 1; h >>= 1) {
        if (u < h) {
            lo[u] = merit_min(lo[u], lo[u + h]);
            hi[u] = merit_max(hi[u], hi[u + h]);
        }
        __syncthreads();
    }
}

// min r, max r of a pair from its chunks' entries ws_range[chunks][3] (entries 1 and 2), by a workgroup of W threads; result in lo[0], hi[0]
template <int W> __device__ __forceinline__ void merit_pair_range(const double *__restrict__ ws_range, int chunks, double *lo, double *hi, int u)
{
    double mn = INFINITY, mx = -INFINITY;
    for (int c = u; c < chunks; c += W) {
        mn = merit_min(mn, ws_range[3 * (size_t)c + 1]);
        mx = merit_max(mx, ws_range[3 * (size_t)c + 2]);
    }
    lo[u] = mn, hi[u] = mx;
    merit_halve_range<W>(lo, hi, u);
}

template <typename T>
__global__ __launch_bounds__(kMeritThreads) void merit_range_kernel(const T *__restrict__ ref, const T *__restrict__ test, MeritShape sh,
                                                                    double *__restrict__ ws)
{
    __shared__ double red[3][kMeritThreads];
    const int u = threadIdx.x;
    const int k = blockIdx.x / sh.chunks, c = blockIdx.x - k * sh.chunks;
    const size_t base = (size_t)k * (size_t)sh.pix;
    const long long i0 = (long long)c * kMeritChunk + u;
    double acc = 0.0, mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
    for (int j = 0; j < kMeritChunk / kMeritThreads; ++j) {
        const long long i = i0 + (long long)j * kMeritThreads;
        if (i < sh.pix) {
            const double r = (double)ref[base + (size_t)i], t = (double)test[base + (size_t)i];
            const double d = r - t;
            acc = acc + d * d;
            mn = merit_min(mn, r);
            mx = merit_max(mx, r);
        }
    }
    red[0][u] = acc, red[1][u] = mn, red[2][u] = mx;
    merit_halve_range<kMeritThreads>(red[1], red[2], u);
    merit_halve_sum<kMeritThreads>(red[0], u);
    if (u < 3) ws[3 * (size_t)blockIdx.x + u] = red[u][0];
}

template <typename T>
__global__ __launch_bounds__(kMeritThreads) void merit_ssim_kernel(const T *__restrict__ ref, const T *__restrict__ test, MeritShape sh,
                                                                   const double *__restrict__ ws_range, double *__restrict__ ws_tiles)
{
    extern __shared__ __align__(16) unsigned char merit_lds[];
    double (*px)[kMeritHalo][kMeritHalo] = reinterpret_cast<double (*)[kMeritHalo][kMeritHalo]>(merit_lds);
    double (*rows)[kMeritHalo][kMeritTile] = reinterpret_cast<double (*)[kMeritHalo][kMeritTile]>(merit_lds + kMeritPxDoubles * sizeof(double));
    double (*red)[kMeritThreads] = reinterpret_cast<double (*)[kMeritThreads]>(merit_lds + (kMeritPxDoubles + kMeritRowDoubles) * sizeof(double));
    const int u = threadIdx.x;
    const int k = blockIdx.x / sh.tiles, b = blockIdx.x - k * sh.tiles;
    const int tr = b / sh.tiles_c, tc = b - tr * sh.tiles_c;
    const int i0 = tr * kMeritTile, j0 = tc * kMeritTile;          // first window position = first pixel of the tile
    const int win = sh.win, edge = kMeritTile + win - 1;
    const size_t base = (size_t)k * (size_t)sh.pix;

    merit_pair_range<kMeritThreads>(ws_range + 3 * (size_t)k * sh.chunks, sh.chunks, red[0], red[1], u);
    const double R = red[1][0] - red[0][0];
    const double a1 = 0.01 * R, a2 = 0.03 * R;
    const double c1 = a1 * a1, c2 = a2 * a2;
    const double NP = (double)(win * win);
    const double cov_norm = NP / (NP - 1.0);

    for (int e = u; e < edge * edge; e += kMeritThreads) {
        const int a = e / edge, q = e - a * edge;
        const int gi = i0 + a, gj = j0 + q;
        double r = 0.0, t = 0.0;
        if (gi < sh.X && gj < sh.Y) {
            const size_t at = base + (size_t)gi * sh.Y + gj;
            r = (double)ref[at], t = (double)test[at];
        }
        px[0][a][q] = r, px[1][a][q] = t;
    }
    __syncthreads();
    // row sums: pixel row a of the tile, window column j
    for (int e = u; e < edge * kMeritTile; e += kMeritThreads) {
        const int a = e / kMeritTile, j = e - a * kMeritTile;
        double r = px[0][a][j], t = px[1][a][j];
        double sr = r, st = t, srr = r * r, stt = t * t, srt = r * t;
        for (int q = 1; q < win; ++q) {
            r = px[0][a][j + q], t = px[1][a][j + q];
            sr = sr + r, st = st + t, srr = srr + r * r, stt = stt + t * t, srt = srt + r * t;
        }
        rows[0][a][j] = sr, rows[1][a][j] = st, rows[2][a][j] = srr, rows[3][a][j] = stt, rows[4][a][j] = srt;
    }
    __syncthreads();
    // window sums and S of positions p = u, u + 256, ... of the tile (row-major), added in that order
    double acc = 0.0;
#pragma unroll 1
    for (int p = u; p < kMeritTile * kMeritTile; p += kMeritThreads) {
        const int i = p / kMeritTile, j = p - i * kMeritTile;
        if (i0 + i < sh.Xo && j0 + j < sh.Yo) {
            double wr = rows[0][i][j], wt = rows[1][i][j], wrr = rows[2][i][j], wtt = rows[3][i][j], wrt = rows[4][i][j];
            for (int a = 1; a < win; ++a) {
                wr = wr + rows[0][i + a][j], wt = wt + rows[1][i + a][j];
                wrr = wrr + rows[2][i + a][j], wtt = wtt + rows[3][i + a][j], wrt = wrt + rows[4][i + a][j];
            }
            const double ux = wr / NP, uy = wt / NP, uxx = wrr / NP, uyy = wtt / NP, uxy = wrt / NP;
            const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
            const double num = ((2.0 * ux) * uy + c1) * ((2.0 * vxy) + c2);
            const double den = ((ux * ux + uy * uy) + c1) * ((vx + vy) + c2);
            acc = acc + num / den;
        }
    }
    __syncthreads();       // (red[] was read for R by every thread before the first barrier above)
    red[0][u] = acc;
    merit_halve_sum<kMeritThreads>(red[0], u);
    if (u == 0) ws_tiles[blockIdx.x] = red[0][0];
}

__global__ __launch_bounds__(kMeritFinishThreads) void merit_finish_kernel(MeritShape sh, const double *__restrict__ ws_range,
                                                                           const double *__restrict__ ws_tiles, double *__restrict__ out)
{
    __shared__ double red[4][kMeritFinishThreads];
    const int u = threadIdx.x, k = blockIdx.x;
    const double *rg = ws_range + 3 * (size_t)k * sh.chunks;
    const double *tl = ws_tiles + (size_t)k * sh.tiles;
    merit_pair_range<kMeritFinishThreads>(rg, sh.chunks, red[2], red[3], u);
    double sq = 0.0, ss = 0.0;
    for (int c = u; c < sh.chunks; c += kMeritFinishThreads) sq = sq + rg[3 * (size_t)c];
    for (int b = u; b < sh.tiles; b += kMeritFinishThreads) ss = ss + tl[b];
    red[0][u] = sq, red[1][u] = ss;
    merit_halve_sum<kMeritFinishThreads>(red[0], u);
    merit_halve_sum<kMeritFinishThreads>(red[1], u);
    if (u == 0) {
        const double R = red[3][0] - red[2][0];
        const double mse = red[0][0] / (double)sh.pix;
        const double ssim = red[1][0] / ((double)sh.Xo * (double)sh.Yo);
        out[3 * (size_t)k] = mse;
        out[3 * (size_t)k + 1] = ssim;
        out[3 * (size_t)k + 2] = mse == 0.0 ? (double)INFINITY : 10.0 * log10((R * R) / mse);
    }
}

static int merit_check(const char *what, int n, int X, int Y)
{
    CTPVAE_REQUIRE(n >= 0, "%s: n must be >= 0 (got %d)", what, n);
    CTPVAE_REQUIRE(X >= 3 && Y >= 3, "%s: images must be at least 3 x 3, the smallest SSIM window (got %d x %d)", what, X, Y);
    CTPVAE_REQUIRE((long long)X * Y <= INT_MAX, "%s: X * Y must fit 31 bits (got %d x %d)", what, X, Y);
    CTPVAE_REQUIRE((long long)n * ((long long)X * Y) <= INT_MAX, "%s: n * X * Y must fit 31 bits (got n=%d, %d x %d)", what, n, X, Y);
    return CTPVAE_OK;
}

template <typename T>
static int merit_launch(const char *what, const T *ref_dev, const T *test_dev, int n, int X, int Y, void *workspace_dev, double *out_dev,
                        ctpvae_stream_t stream)
{
    static std::atomic<unsigned long long> attr_set{0};      // one per instantiation
    if (int rc = merit_check(what, n, X, Y)) return rc;
    if (n == 0) return CTPVAE_OK;
    CTPVAE_REQUIRE(ref_dev && test_dev && workspace_dev && out_dev, "%s: null pointer", what);
    CTPVAE_REQUIRE(((size_t)workspace_dev & 7) == 0 && ((size_t)out_dev & 7) == 0 && ((size_t)ref_dev & (sizeof(T) - 1)) == 0 &&
                   ((size_t)test_dev & (sizeof(T) - 1)) == 0, "%s: images must be aligned to their element, workspace and out to 8 bytes", what);
    const MeritShape sh = merit_shape(n, X, Y);
    double *ws_range = static_cast<double *>(workspace_dev);                   // [n][chunks][3]
    double *ws_tiles = ws_range + 3 * (size_t)n * sh.chunks;                   // [n][tiles]
    // n * chunks and n * tiles are both <= n * X * Y <= 2^31 - 1, a grid's x limit
    CTPVAE_SET_MAX_LDS_ONCE(merit_ssim_kernel<T>, attr_set);
    hipLaunchKernelGGL(merit_range_kernel<T>, dim3((unsigned)n * sh.chunks), dim3(kMeritThreads), 0, (hipStream_t)stream, ref_dev, test_dev, sh,
                       ws_range);
    CTPVAE_LAUNCH_CHECK("merit_range_kernel");
    hipLaunchKernelGGL(merit_ssim_kernel<T>, dim3((unsigned)n * sh.tiles), dim3(kMeritThreads), kMeritSsimLdsBytes, (hipStream_t)stream, ref_dev, test_dev, sh,
                       ws_range, ws_tiles);
    CTPVAE_LAUNCH_CHECK("merit_ssim_kernel");
    hipLaunchKernelGGL(merit_finish_kernel, dim3((unsigned)n), dim3(kMeritFinishThreads), 0, (hipStream_t)stream, sh, ws_range, ws_tiles, out_dev);
    CTPVAE_LAUNCH_CHECK("merit_finish_kernel");
    return CTPVAE_OK;
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

int ctpvae_merit_tile(void) { return kMeritTile; }

long long ctpvae_merit_workspace_bytes(int n, int X, int Y)
{
    if (int rc = merit_check("merit_workspace_bytes", n, X, Y)) return rc;
    const MeritShape sh = merit_shape(n, X, Y);
    return (long long)n * (3ll * sh.chunks + sh.tiles) * (long long)sizeof(double);
}

int ctpvae_merit_f32(const float *ref_dev, const float *test_dev, int n, int X, int Y, void *workspace_dev, double *out_dev,
                     ctpvae_stream_t stream)
{
    return merit_launch<float>("merit_f32", ref_dev, test_dev, n, X, Y, workspace_dev, out_dev, stream);
}

int ctpvae_merit_f64(const double *ref_dev, const double *test_dev, int n, int X, int Y, void *workspace_dev, double *out_dev,
                     ctpvae_stream_t stream)
{
    return merit_launch<double>("merit_f64", ref_dev, test_dev, n, X, Y, workspace_dev, out_dev, stream);
}

}  // extern "C"
