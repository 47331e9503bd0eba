// The reference's offline face extraction (dataset/generate_dataset.py:53-91 with dataset/dataset.py:152-181, 191-239, 127-139) for its
// un-augmented variant, on the device: per face, the rotation-removing warp of the face rectangle out of the decoded source image and
// Pillow's 8-bit bilinear resampling of that rectangle to out x out.  Semantics under cg_faces_u8_extract in catgan.h; the numpy
// restatement is faces.extract_faces_np.  Two kernels:
//   faces_warp_hpass_k  one workgroup per band of rectangle rows of one face: the rows are warped into the LDS as bytes (only rectangle
//                       pixels are ever warped - the warp is pointwise, so this equals rotating the whole image and cropping), then
//                       the horizontal pass runs out of the LDS against the face's taps into tmp[face][row][out][3];
//   faces_vpass_k       the vertical pass, consecutive lanes along (ox, c): loads and stores are contiguous.
// Nothing but tmp (Hr out 3 bytes per face) goes to memory between them.  The warp is fp32 with every operation rounded once, the
// resampling is integer arithmetic alone: no floating point decides a tap on the device.
#include <vector>
#include "common.h"

namespace cg {
namespace {

constexpr int kBandBytes = 32768;   // the LDS a workgroup keeps its warped rows in
constexpr int kBandRowsMax = 16;
constexpr int kGeom = 8;            // int32 per face: Hs Ws y0 x0 Hr Wr kx ky
// rows per band of a rectangle Wr wide: >= 2 for every Wr <= 4096
__host__ __device__ inline int band_rows(int Wr) {
    const int r = kBandBytes / (Wr * 3);
    return r > kBandRowsMax ? kBandRowsMax : r;
}
// Pillow's ksize of one axis (Resample.c precompute_coeffs, bilinear support 1): 2 ceil(max(in / out, 1)) + 1
inline int resample_ksize(int in, int out) { return 2 * ((std::max(in, out) + out - 1) / out) + 1; }
__device__ __forceinline__ unsigned char clip8(int ss) {
    const int v = ss >> 22;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ void __launch_bounds__(256) faces_warp_hpass_k(const unsigned char* __restrict__ src, const uint64_t* __restrict__ src_off,
                                                          const int32_t* __restrict__ geom, const float* __restrict__ inv,
                                                          const int32_t* __restrict__ taps, const uint64_t* __restrict__ tap_off,
                                                          const int32_t* __restrict__ band_start, const uint64_t* __restrict__ tmp_off,
                                                          unsigned char* __restrict__ tmp, int N, int out) {
#pragma clang fp contract(off)
    __shared__ unsigned char band[kBandBytes];   // [rows][Wr][3]
    __shared__ float unit[256];                  // u8 / 255, divided once per workgroup and not twelve times per pixel
    unit[threadIdx.x] = __fdiv_rn((float)threadIdx.x, 255.f);
    __syncthreads();
    const int b = blockIdx.x;
    int f = 0, hi = N;                           // the face whose bands hold b: band_start[f] <= b < band_start[f + 1]
    while (hi - f > 1) {
        const int mid = (f + hi) >> 1;
        if (band_start[mid] <= b) f = mid; else hi = mid;
    }
    const int32_t* g = geom + (long)f * kGeom;
    const int Hs = g[0], Ws = g[1], y0 = g[2], x0 = g[3], Hr = g[4], Wr = g[5], kx = g[6];
    const int R = band_rows(Wr), r0 = (b - band_start[f]) * R, nr = min(R, Hr - r0);
    const unsigned char* im = src + src_off[f];
    const float* m = inv + (long)f * 6;
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const int row3 = Ws * 3;
    for (int e = threadIdx.x; e < nr * Wr; e += 256) {
        const int r = e / Wr, x = e - r * Wr;
        const float xf = (float)(x0 + x), yf = (float)(y0 + r0 + r);
        const float ax = m00 * xf, bx = m01 * yf, ay = m10 * xf, by = m11 * yf;
        int tx0, tx1, ty0, ty1;
        float fx, fy;
        warp_taps((ax + bx) + m02, Ws, &tx0, &tx1, &fx);
        warp_taps((ay + by) + m12, Hs, &ty0, &ty1, &fy);
        const float gx = 1.f - fx, gy = 1.f - fy;
        const unsigned char *p00 = im + ty0 * row3 + tx0 * 3, *p01 = im + ty0 * row3 + tx1 * 3;
        const unsigned char *p10 = im + ty1 * row3 + tx0 * 3, *p11 = im + ty1 * row3 + tx1 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float ta = gx * unit[p00[c]], tb = fx * unit[p01[c]], ba = gx * unit[p10[c]], bb = fx * unit[p11[c]];
            const float top = ta + tb, bot = ba + bb;
            const float wa = gy * top, wb = fy * bot;
            band[e * 3 + c] = (unsigned char)(int)((wa + wb) * 255.f);   // dataset.py:174 truncates
        }
    }
    __syncthreads();
    const int32_t* tb = taps + tap_off[2 * f];   // [out][2] (xmin, count), then [out][kx] taps
    const int32_t* tk = tb + 2 * out;
    const int o3 = out * 3;
    unsigned char* trow = tmp + tmp_off[f] + (long)r0 * o3;
    for (int e = threadIdx.x; e < nr * o3; e += 256) {
        const int r = e / o3, j = e - r * o3, ox = j / 3, c = j - ox * 3;
        const int xmin = tb[2 * ox], cnt = tb[2 * ox + 1];
        const unsigned char* p = band + (r * Wr + xmin) * 3 + c;
        const int32_t* k = tk + ox * kx;
        int ss = 1 << 21;
#pragma unroll 1
        for (int i = 0; i < cnt; ++i) ss += (int)p[i * 3] * k[i];
        trow[e] = clip8(ss);
    }
}

__global__ void __launch_bounds__(256) faces_vpass_k(const unsigned char* __restrict__ tmp, const uint64_t* __restrict__ tmp_off,
                                                     const int32_t* __restrict__ geom, const int32_t* __restrict__ taps,
                                                     const uint64_t* __restrict__ tap_off, unsigned char* __restrict__ dst, int out,
                                                     int blocks_per_face) {
    const int f = blockIdx.x / blocks_per_face;
    const int e = (blockIdx.x - f * blocks_per_face) * 256 + threadIdx.x;
    const int o3 = out * 3;
    if (e >= out * o3) return;
    const int oy = e / o3, j = e - oy * o3;
    const int ky = geom[(long)f * kGeom + 7];
    const int32_t* tb = taps + tap_off[2 * f + 1];
    const int32_t* k = tb + 2 * out + oy * ky;
    const int ymin = tb[2 * oy], cnt = tb[2 * oy + 1];
    const unsigned char* p = tmp + tmp_off[f] + (long)ymin * o3 + j;
    int ss = 1 << 21;
    for (int i = 0; i < cnt; ++i) ss += (int)p[(long)i * o3] * k[i];
    dst[(long)f * out * o3 + e] = clip8(ss);
}

// one axis' table at taps + off: inside the array, every sample's taps inside the side
int check_table(const std::vector<int32_t>& taps, uint64_t off, int in, int out, int ksize, int f, const char* axis) {
    CG_REQUIRE(off <= taps.size() && (uint64_t)out * (2 + ksize) <= taps.size() - off,
               "cg_faces_u8_extract: face %d: the %s tap table at %llu does not fit the %zu taps given", f, axis, (unsigned long long)off, taps.size());
    const int32_t* tb = taps.data() + off;
    for (int o = 0; o < out; ++o) {
        const long lo = tb[2 * o], cnt = tb[2 * o + 1];
        CG_REQUIRE(lo >= 0 && cnt >= 0 && cnt <= ksize && lo + cnt <= in,
                   "cg_faces_u8_extract: face %d: %s sample %d reads [%ld, %ld) of a side of %d with ksize %d", f, axis, o, lo, lo + cnt, in, ksize);
    }
    return 0;
}

}  // namespace
}  // namespace cg

using namespace cg;

int cg_faces_u8_extract(void* stream, const unsigned char* src, size_t src_bytes, const uint64_t* src_off, const int32_t* geom,
                        const float* inv, const int32_t* taps, size_t ntaps, const uint64_t* tap_off, unsigned char* dst, int N, int out,
                        void* workspace, size_t workspace_bytes) {
    CG_REQUIRE(src && src_off && geom && inv && taps && tap_off && dst && workspace, "cg_faces_u8_extract: null pointer");
    CG_REQUIRE(N > 0 && N <= (1 << 20), "cg_faces_u8_extract: N = %d is outside 1..2^20", N);
    CG_REQUIRE(out >= 8 && out <= 128, "cg_faces_u8_extract: out = %d is outside 8..128", out);
    CG_REQUIRE(src_bytes > 0 && ntaps > 0 && ntaps <= (size_t)1 << 28, "cg_faces_u8_extract: bad array lengths (%zu source bytes, %zu taps)", src_bytes, ntaps);
    hipStream_t s = S(stream);
    // the descriptors are device arrays: they come back once, so that every limit is checked before anything is launched
    std::vector<int32_t> hgeom((size_t)N * kGeom), htaps(ntaps);
    std::vector<uint64_t> hsrc(N), htap((size_t)N * 2);
    CG_HIP(hipMemcpyAsync(hgeom.data(), geom, hgeom.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CG_HIP(hipMemcpyAsync(htaps.data(), taps, htaps.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CG_HIP(hipMemcpyAsync(hsrc.data(), src_off, hsrc.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    CG_HIP(hipMemcpyAsync(htap.data(), tap_off, htap.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    CG_HIP(hipStreamSynchronize(s));
    // workspace: band_start [N + 1] int32 | tmp_off [N] uint64 | tmp bytes
    const size_t off_tmpoff = ((size_t)(N + 1) * 4 + 15) / 16 * 16, off_tmp = (off_tmpoff + (size_t)N * 8 + 15) / 16 * 16;
    std::vector<unsigned char> head(off_tmp, 0);
    int32_t* band_start = reinterpret_cast<int32_t*>(head.data());
    uint64_t* tmp_off = reinterpret_cast<uint64_t*>(head.data() + off_tmpoff);
    long bands = 0;
    uint64_t rows = 0;
    for (int f = 0; f < N; ++f) {
        const int32_t* g = hgeom.data() + (size_t)f * kGeom;
        const int Hs = g[0], Ws = g[1], y0 = g[2], x0 = g[3], Hr = g[4], Wr = g[5], kx = g[6], ky = g[7];
        CG_REQUIRE(Hs >= 8 && Hs <= 8192 && Ws >= 8 && Ws <= 8192, "cg_faces_u8_extract: face %d: a %d x %d source is outside 8..8192", f, Ws, Hs);
        CG_REQUIRE(Hr >= 8 && Hr <= 4096 && Wr >= 8 && Wr <= 4096, "cg_faces_u8_extract: face %d: a %d x %d rectangle is outside 8..4096", f, Wr, Hr);
        CG_REQUIRE(y0 >= 0 && x0 >= 0 && (long)y0 + Hr <= Hs && (long)x0 + Wr <= Ws,
                   "cg_faces_u8_extract: face %d: the rectangle (%d, %d) + %d x %d is not inside its %d x %d source", f, x0, y0, Wr, Hr, Ws, Hs);
        CG_REQUIRE(hsrc[f] <= src_bytes && (uint64_t)Hs * Ws * 3 <= src_bytes - hsrc[f],
                   "cg_faces_u8_extract: face %d: its source at %llu does not fit the %zu bytes given", f, (unsigned long long)hsrc[f], src_bytes);
        CG_REQUIRE(kx == resample_ksize(Wr, out) && ky == resample_ksize(Hr, out),
                   "cg_faces_u8_extract: face %d: ksize (%d, %d) disagrees with the sides %d x %d -> %d, which need (%d, %d)", f, kx, ky, Wr, Hr, out,
                   resample_ksize(Wr, out), resample_ksize(Hr, out));
        if (int rc = check_table(htaps, htap[2 * f], Wr, out, kx, f, "horizontal")) return rc;
        if (int rc = check_table(htaps, htap[2 * f + 1], Hr, out, ky, f, "vertical")) return rc;
        band_start[f] = (int32_t)bands;
        tmp_off[f] = rows * (uint64_t)out * 3;
        bands += cdiv(Hr, band_rows(Wr));
        rows += (uint64_t)Hr;
    }
    band_start[N] = (int32_t)bands;
    CG_REQUIRE(bands <= INT32_MAX, "cg_faces_u8_extract: %ld bands of rows do not fit one launch", bands);
    const size_t need = off_tmp + rows * (size_t)out * 3;
    CG_REQUIRE(workspace_bytes >= need, "cg_faces_u8_extract: the workspace has %zu bytes, %zu are needed", workspace_bytes, need);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    CG_HIP(hipMemcpyAsync(ws, head.data(), head.size(), hipMemcpyHostToDevice, s));
    CG_HIP(hipStreamSynchronize(s));   // `head` is pageable and ends with this call
    hipLaunchKernelGGL(faces_warp_hpass_k, dim3((unsigned)bands), dim3(256), 0, s, src, src_off, geom, inv, taps, tap_off,
                       reinterpret_cast<const int32_t*>(ws), reinterpret_cast<const uint64_t*>(ws + off_tmpoff), ws + off_tmp, N, out);
    CG_LAUNCH_CHECK();
    const int bpf = cdiv((long)out * out * 3, 256);
    hipLaunchKernelGGL(faces_vpass_k, dim3((unsigned)(N * (long)bpf)), dim3(256), 0, s, ws + off_tmp,
                       reinterpret_cast<const uint64_t*>(ws + off_tmpoff), geom, taps, tap_off, dst, out, bpf);
    CG_LAUNCH_CHECK();
    return 0;
}
