// SIFT extraction kernels for gfx950.  Every grid spans the
// batch (one 640 x 480 image cannot fill the device); the arithmetic is
// sift_point.h's, the same statements as the host twin in sift.cpp.
//   smoothing    a column pass and a row pass per level through LDS tiles of
//                64 x 16 outputs plus the halo, float, taps from the host
//   detection    one workgroup per (row, DoG level, image): the fused DoG +
//                extremum + refinement test of each cell, run once to count
//                and, after a scan of the row counts, once more to write the
//                keypoints at their place in (level, row, column) order.  No
//                atomics: the order is fixed by the scan.
//   gradient     magnitude and angle of the S levels keypoints live in
//   orientation  one wavefront per keypoint: the lanes compute 64 samples at
//                a time into LDS, then lane b < 36 walks them in sample order
//                and adds what falls into bin b, so every bin's sum is taken
//                in row-major sample order, as the host twin takes it
//   descriptor   one wavefront per (keypoint, orientation): the same shape,
//                lane l owning bins 2l and 2l + 1 of the 128; lane 0 finishes
// No floating-point atomics anywhere.
#pragma clang fp contract(off)

#include "common.h"
#include "sift.h"

namespace sfm {
using namespace sift;

namespace {

__global__ __launch_bounds__(256) void sift_u8_kernel(const uint8_t* __restrict__ g, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)g[i];
}

__global__ __launch_bounds__(256) void sift_decimate_kernel(const float* __restrict__ src, int ws, int hs,
                                                            float* __restrict__ dst, int w, int h) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)w * h) return;
    const int x = (int)(i % w), y = (int)(i / w);
    const int img = blockIdx.y;
    dst[(int64_t)img * w * h + i] = src[(int64_t)img * ws * hs + (int64_t)(2 * y) * ws + 2 * x];
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// DIR 0: along y (columns), DIR 1: along x (rows)
template <int DIR>
__global__ __launch_bounds__(256) void sift_conv_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                        const float* __restrict__ taps, int W, int w, int h) {
    __shared__ float tile[(kSiftTileY + 2 * kMaxHalf) * kSiftTileX];
    __shared__ float tp[2 * kMaxHalf + 1];
    const int tid = threadIdx.x, x0 = blockIdx.x * kSiftTileX, y0 = blockIdx.y * kSiftTileY;
    const int64_t wh = (int64_t)w * h;
    src += blockIdx.z * wh;
    dst += blockIdx.z * wh;
    if (tid <= 2 * W) tp[tid] = taps[tid];
    const int pitch = DIR == 0 ? kSiftTileX : kSiftTileX + 2 * W;
    const int rows = DIR == 0 ? kSiftTileY + 2 * W : kSiftTileY;
    for (int i = tid; i < rows * pitch; i += 256) {
        const int r = i / pitch, c = i % pitch;
        const int yy = DIR == 0 ? clampi(y0 - W + r, 0, h - 1) : clampi(y0 + r, 0, h - 1);
        const int xx = DIR == 0 ? clampi(x0 + c, 0, w - 1) : clampi(x0 - W + c, 0, w - 1);
        tile[i] = src[(int64_t)yy * w + xx];
    }
    __syncthreads();
    const int tx = tid & 63, x = x0 + tx;
    for (int oy = tid >> 6; oy < kSiftTileY; oy += 4) {
        const int y = y0 + oy;
        if (x >= w || y >= h) continue;
        float acc;
        if (DIR == 0) acc = conv_acc([&](int j) { return tile[(oy + j) * kSiftTileX + tx]; }, tp, W);
        else acc = conv_acc([&](int j) { return tile[oy * pitch + tx + j]; }, tp, W);
        dst[(int64_t)y * w + x] = acc;
    }
}

__device__ inline Levels image_levels(const SiftOctave& o, int img) {
    Levels lv;
    const int64_t off = (int64_t)img * o.w * o.h;
    for (int i = 0; i < kMaxLevels; ++i) lv.L[i] = i < o.S + 3 ? o.lv.L[i] + off : nullptr;
    return lv;
}

// one workgroup per (row y = blockIdx.x + 1, level k = blockIdx.y + 1, image)
template <bool WRITE>
__global__ __launch_bounds__(256) void sift_detect_kernel(SiftOctave o) {
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int y = blockIdx.x + 1, k = blockIdx.y + 1, img = blockIdx.z;
    const Levels lv = image_levels(o, img);
    const int64_t slot = (int64_t)img * o.S * o.h + (int64_t)(k - 1) * o.h + y;
    const int base = WRITE ? o.rowbase[slot] : 0;
    int running = 0;
    for (int xs = 1; xs < o.w - 1; xs += 256) {
        const int x = xs + tid;
        Keypoint kp;
        const bool good = x < o.w - 1 && detect_cell(lv, o.w, o.h, o.S, x, y, k, o.tp, o.te, o.sigma0, o.xper, &kp);
        const unsigned long long m = __ballot(good);
        if (lane == 0) wtot[wv] = __popcll(m);
        __syncthreads();
        int pre = 0, tot = 0;
        for (int i = 0; i < 4; ++i) {
            pre += i < wv ? wtot[i] : 0;
            tot += wtot[i];
        }
        if (WRITE && good) {
            const int at = base + running + pre + __popcll(m & ((1ull << lane) - 1ull));
            if (at < o.kcap) o.kps[(int64_t)img * o.kcap + at] = kp;
        }
        running += tot;
        __syncthreads();
    }
    if (!WRITE && tid == 0) o.rowcnt[slot] = running;
}

// out[i] = add + (in[0] + .. + in[i-1]) per image, one workgroup per image;
// total[img] = the sum; accum[img] (optional) is read as `add` and advanced
__global__ __launch_bounds__(256) void sift_scan_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                        int64_t stride, const int32_t* __restrict__ n_per,
                                                        int32_t n_fixed, int32_t* __restrict__ total,
                                                        int32_t* __restrict__ accum) {
    __shared__ int part[256];
    const int tid = threadIdx.x, img = blockIdx.x;
    const int n = n_per ? n_per[img] : n_fixed;
    in += img * stride;
    out += img * stride;
    const int add = accum ? accum[img] : 0;
    const int per = (n + 255) / 256;
    const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += in[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = add + part[tid] - sum;
    for (int i = lo; i < hi; ++i) {
        const int v = in[i];
        out[i] = run;
        run += v;
    }
    if (tid == 255) {
        total[img] = part[255];
        if (accum) accum[img] = add + part[255];
    }
}

__global__ __launch_bounds__(256) void sift_grad_kernel(SiftOctave o) {
    const int64_t wh = (int64_t)o.w * o.h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= wh) return;
    const int k = blockIdx.y + 1, img = blockIdx.z;
    float mod, ang;
    gradient(o.lv.L[k] + img * wh, o.w, o.h, (int)(i % o.w), (int)(i / o.w), mod, ang);
    float* g = o.grad + ((int64_t)img * o.S + (k - 1)) * 2 * wh + 2 * i;
    g[0] = mod;
    g[1] = ang;
}

__device__ inline const float* grad_level(const SiftOctave& o, int img, int k) {
    return o.grad + ((int64_t)img * o.S + (k - 1)) * 2 * (int64_t)o.w * o.h;
}

// one wavefront per keypoint
__global__ __launch_bounds__(64) void sift_orient_kernel(SiftOctave o) {
    __shared__ double hist[kOriBins];
    __shared__ double sw0[64], sw1[64];
    __shared__ int sbin[64];
    const int lane = threadIdx.x, q = blockIdx.x, img = blockIdx.y;
    if (q >= o.ktot[img] || q >= o.kcap) return;
    const int64_t slot = (int64_t)img * o.kcap + q;
    if (!o.orientation) {
        if (lane == 0) o.nang[slot] = 1;
        if (lane < 4) o.angles[4 * slot + lane] = 0.0;
        return;
    }
    const Keypoint kp = o.kps[slot];
    const OriWindow win = ori_window(kp, o.xper, o.w, o.h);
    if (!win.ok) {
        if (lane == 0) o.nang[slot] = 0;
        return;
    }
    const float* grad = grad_level(o, img, kp.k);
    const int nx = win.x1 - win.x0 + 1, ny = win.y1 - win.y0 + 1, total = nx * ny;
    double acc = 0.0;
    for (int base = 0; base < total; base += 64) {
        const int i = base + lane;
        int bin = -1;
        double w0 = 0.0, w1 = 0.0;
        if (i < total && !ori_sample(win, grad, o.w, o.expn, win.x0 + i % nx, win.y0 + i / nx, bin, w0, w1)) bin = -1;
        sbin[lane] = bin;
        sw0[lane] = w0;
        sw1[lane] = w1;
        __syncthreads();
        const int cnt = total - base < 64 ? total - base : 64;
        for (int j = 0; j < cnt; ++j) {
            const int b = sbin[j];
            if (b < 0) continue;
            if (b == lane) acc += sw0[j];
            else if ((b + 1) % kOriBins == lane) acc += sw1[j];
        }
        __syncthreads();
    }
    if (lane < kOriBins) hist[lane] = acc;
    __syncthreads();
    if (lane == 0) {
        double ang[4] = {0, 0, 0, 0};
        const int n = ori_peaks(hist, ang);
        o.nang[slot] = n;
        for (int a = 0; a < 4; ++a) o.angles[4 * slot + a] = ang[a];
    }
}

// one wavefront per (keypoint, orientation)
__global__ __launch_bounds__(64) void sift_desc_kernel(SiftOctave o) {
    __shared__ DescSample ss[64];
    __shared__ float dd[128];
    const int lane = threadIdx.x, q = blockIdx.x >> 2, a = blockIdx.x & 3, img = blockIdx.y;
    if (q >= o.ktot[img] || q >= o.kcap) return;
    const int64_t slot = (int64_t)img * o.kcap + q;
    if (a >= o.nang[slot]) return;
    const int64_t row = (int64_t)o.row[slot] + a;
    if (row >= o.cap) return;
    const Keypoint kp = o.kps[slot];
    const double angle = o.angles[4 * slot + a];
    const DescWindow d = desc_window(kp, angle, o.xper, o.w, o.h);
    const int my_by = (lane >> 4) - 2, my_bx = ((lane >> 2) & 3) - 2, my_bt = (lane & 3) * 2;
    float acc0 = 0.f, acc1 = 0.f;
    const int nx = d.x1 - d.x0 + 1, ny = d.y1 - d.y0 + 1;
    if (d.ok && nx > 0 && ny > 0) {
        const float* grad = grad_level(o, img, kp.k);
        const int total = nx * ny;
        for (int base = 0; base < total; base += 64) {
            const int i = base + lane;
            if (i < total) ss[lane] = desc_sample(d, grad, o.w, o.expn, d.x0 + i % nx, d.y0 + i / nx);
            __syncthreads();
            const int cnt = total - base < 64 ? total - base : 64;
            for (int j = 0; j < cnt; ++j) {
                const DescSample s = ss[j];
                const int dbx = my_bx - s.bx, dby = my_by - s.by;
                if ((unsigned)dbx < 2u && (unsigned)dby < 2u) {
                    const int t0 = (my_bt - s.bt) & 7, t1 = (my_bt + 1 - s.bt) & 7;
                    if (t0 < 2) acc0 += desc_weight(s, dbx, dby, t0);
                    if (t1 < 2) acc1 += desc_weight(s, dbx, dby, t1);
                }
            }
            __syncthreads();
        }
    }
    dd[2 * lane] = acc0;
    dd[2 * lane + 1] = acc1;
    __syncthreads();
    if (lane == 0) {
        desc_finish(dd, o.root_sift, o.desc + ((int64_t)img * o.cap + row) * 128);
        float* f = o.xyso + ((int64_t)img * o.cap + row) * 4;
        f[0] = kp.x;
        f[1] = kp.y;
        f[2] = kp.sigma;
        f[3] = (float)angle;
    }
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void sift_launch_u8(const uint8_t* gray, float* out, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sift_u8_kernel, dim3(blocks_of(n)), dim3(256), 0, s, gray, out, n);
    SFM_HIP(hipGetLastError());
}

void sift_launch_decimate(const float* src, int ws, int hs, float* dst, int w, int h, int n_img, hipStream_t s) {
    hipLaunchKernelGGL(sift_decimate_kernel, dim3(blocks_of((int64_t)w * h), n_img), dim3(256), 0, s, src, ws, hs, dst,
                       w, h);
    SFM_HIP(hipGetLastError());
}

void sift_launch_smooth(const float* src, float* tmp, float* dst, const float* taps, int W, int w, int h, int n_img,
                        hipStream_t s) {
    const dim3 grid((w + kSiftTileX - 1) / kSiftTileX, (h + kSiftTileY - 1) / kSiftTileY, n_img);
    hipLaunchKernelGGL(sift_conv_kernel<0>, grid, dim3(256), 0, s, src, tmp, taps, W, w, h);
    hipLaunchKernelGGL(sift_conv_kernel<1>, grid, dim3(256), 0, s, (const float*)tmp, dst, taps, W, w, h);
    SFM_HIP(hipGetLastError());
}

void sift_launch_count(const SiftOctave& o, hipStream_t s) {
    SFM_HIP(hipMemsetAsync(o.rowcnt, 0, sizeof(int32_t) * (size_t)o.n_img * o.S * o.h, s));
    hipLaunchKernelGGL(sift_detect_kernel<false>, dim3(o.h - 2, o.S, o.n_img), dim3(256), 0, s, o);
    hipLaunchKernelGGL(sift_scan_kernel, dim3(o.n_img), dim3(256), 0, s, (const int32_t*)o.rowcnt, o.rowbase,
                       (int64_t)o.S * o.h, (const int32_t*)nullptr, o.S * o.h, o.ktot, (int32_t*)nullptr);
    SFM_HIP(hipGetLastError());
}

void sift_launch_describe(const SiftOctave& o, int32_t kmax, hipStream_t s) {
    if (kmax <= 0) return;
    hipLaunchKernelGGL(sift_detect_kernel<true>, dim3(o.h - 2, o.S, o.n_img), dim3(256), 0, s, o);
    hipLaunchKernelGGL(sift_grad_kernel, dim3(blocks_of((int64_t)o.w * o.h), o.S, o.n_img), dim3(256), 0, s, o);
    hipLaunchKernelGGL(sift_orient_kernel, dim3(kmax, o.n_img), dim3(64), 0, s, o);
    // nang of the slots past an image's count is never read: n_per bounds the scan
    hipLaunchKernelGGL(sift_scan_kernel, dim3(o.n_img), dim3(256), 0, s, (const int32_t*)o.nang, o.row,
                       (int64_t)o.kcap, (const int32_t*)o.ktot, 0, o.ktot + o.n_img, o.ftot);
    hipLaunchKernelGGL(sift_desc_kernel, dim3(4 * (unsigned)kmax, o.n_img), dim3(64), 0, s, o);
    SFM_HIP(hipGetLastError());
}

}  // namespace sfm
