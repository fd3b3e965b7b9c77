// Four-index basis rotations on the FP64 matrix cores, one index at a time.
//   K3/K14  quarter transform (v_mfma_f64_16x16x4_f64)          electron_integral_utils.py:136,
//                                                              gradients_loewdin.py:224-232,339
// The fused two-index steps of the compressed pipeline: pair_transform.hip, pair_pipe.hip, pair_dma.hip, pair64.hip.
// blockIdx.y = geometry of the batch (kernels.hpp).
#include "common.hpp"
#include "kernels.hpp"

namespace evc {

// ------------------------------------------------------------------ quarter transform
// out[q][row] = sum_d in[row][d] * C[d][q],  row = (a,b,c) flattened, rows = n^3.
// MFMA roles: M <-> q (rotated index, C from LDS), N <-> row (16 tensor rows per wave step),
// K <-> d.  Rows of `in` are n contiguous doubles, so the 16 rows a wave consumes form one
// contiguous 16*n*8-byte block; the output is written as 128-byte row segments.
// The first tile's operand loads are issued before the LDS fill of C so both latencies overlap.
template <int NPAD>
__global__ __launch_bounds__(256) void qt_kernel(const double *__restrict__ in, int64_t sin,
                                                 const double *__restrict__ C, int64_t sC, int ct, int n,
                                                 int64_t rows, double *__restrict__ out, int64_t sout) {
    constexpr int LDX = (NPAD % 32 == 0) ? NPAD + 16 : NPAD;  // keeps the two 16-lane halves on disjoint banks
    constexpr int KSTEPS = NPAD / 4;
    constexpr int NT = NPAD / 16;
    __shared__ double Xs[NPAD * LDX];
    in += (int64_t)blockIdx.y * sin;
    C += (int64_t)blockIdx.y * sC;
    out += (int64_t)blockIdx.y * sout;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int64_t ntiles = (rows + 15) / 16;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    double b[KSTEPS];
    {
        const int64_t row = tile * 16 + l15;
        const bool rok = tile < ntiles && row < rows;
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) {
            const int d = 4 * kk + l4;
            b[kk] = (rok && d < n) ? in[row * n + d] : 0.0;
        }
    }
    for (int idx = threadIdx.x; idx < NPAD * NPAD; idx += 256) {
        const int d = idx / NPAD, q = idx % NPAD;
        double v = 0.0;
        if (d < n && q < n) v = ct ? C[q * n + d] : C[d * n + q];
        Xs[d * LDX + q] = v;
    }
    __syncthreads();
    while (tile < ntiles) {
        const int64_t row = tile * 16 + l15;
        const bool rok = row < rows;
        const int64_t next = tile + (int64_t)gridDim.x * 4;
        double bn[KSTEPS];
        {
            const int64_t nrow = next * 16 + l15;
            const bool nok = next < ntiles && nrow < rows;
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) {
                const int d = 4 * kk + l4;
                bn[kk] = (nok && d < n) ? in[nrow * n + d] : 0.0;
            }
        }
        // the NT output tiles are independent accumulation chains: interleave them (a dependent
        // f64 MFMA costs ~3x the issue interval)
        d4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = mfma_f64(Xs[(4 * kk + l4) * LDX + t * 16 + l15], b[kk], acc[t]);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = t * 16 + l4 + 4 * r;
                if (rok && q < n) out[(int64_t)q * rows + row] = acc[t][r];
            }
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) b[kk] = bn[kk];
        tile = next;
    }
}

// Grid: every workgroup stages X (up to 41 KB of LDS) before its first tile, so the launch wants PERSISTENT workgroups --
// one resident round of the chip (the register budget of these kernels allows one wave per SIMD from 64 padded columns
// on, two at 48, four below), each walking many tiles with the next tile's rows in flight -- not one workgroup per four
// tiles (measured per quarter step, one geometry: n = 58 93 -> 48 us, n = 64 133 -> 66 us; a two-tile variant with
// 16-byte operand loads added nothing on top and was dropped).
template <int NPAD>
static int qt_launch(const double *in, int64_t sin, const double *C, int64_t sC, int ct, int n, double *out,
                     int64_t sout, int count, hipStream_t st) {
    const int64_t rows = (int64_t)n * n * n;
    constexpr int kResident = 256 * (NPAD >= 64 ? 1 : NPAD >= 48 ? 2 : 4);   // workgroups of one round
    const int64_t share = (kResident + count - 1) / count;                   // per geometry of the batch
    const int64_t ntiles = (rows + 15) / 16;
    int64_t blocks = (ntiles + 3) / 4;
    if (blocks > share) blocks = share;
    hipLaunchKernelGGL(qt_kernel<NPAD>, dim3((unsigned)blocks, (unsigned)count), dim3(256), 0, st, in, sin, C, sC, ct,
                       n, rows, out, sout);
    EVC_LAUNCH_CHECK("quarter_transform");
    note_kernel(EVC_PROF_PAIR_TRANSFORM, "qt_kernel<%d>", NPAD);
    return 0;
}

int launch_quarter_transform(const double *in, int64_t sin, const double *C, int64_t sC, int ct, int n, double *out,
                             int64_t sout, int count, hipStream_t st) {
    const int npad = (n + 15) / 16 * 16;
    switch (npad) {
        case 16: return qt_launch<16>(in, sin, C, sC, ct, n, out, sout, count, st);
        case 32: return qt_launch<32>(in, sin, C, sC, ct, n, out, sout, count, st);
        case 48: return qt_launch<48>(in, sin, C, sC, ct, n, out, sout, count, st);
        case 64: return qt_launch<64>(in, sin, C, sC, ct, n, out, sout, count, st);
        case 80: return qt_launch<80>(in, sin, C, sC, ct, n, out, sout, count, st);
        case 96: return qt_launch<96>(in, sin, C, sC, ct, n, out, sout, count, st);
        default: break;
    }
    set_error("quarter_transform: n=%d not supported (1..96)", n);
    return -1;
}

}  // namespace evc

// ------------------------------------------------------------------ C ABI
using namespace evc;

extern "C" int evc_quarter_transform(const double *in, const double *C, int c_transposed, int n, double *out,
                                     void *stream) {
    EVC_REQUIRE(in && C && out, "evc_quarter_transform: null pointer");
    EVC_REQUIRE(n >= 1 && n <= 96, "evc_quarter_transform: n=%d out of range 1..96", n);
    EVC_REQUIRE(in != out, "evc_quarter_transform: in and out must not alias");
    return launch_quarter_transform(in, 0, C, 0, c_transposed, n, out, 0, 1, as_stream(stream));
}

extern "C" int evc_four_index_transform(const double *in, const double *C, int c_transposed, int n, double *out,
                                        double *tmp, double *three_quarter, void *stream) {
    EVC_REQUIRE(in && C && out && tmp, "evc_four_index_transform: null pointer");
    EVC_REQUIRE(n >= 1 && n <= 96, "evc_four_index_transform: n=%d out of range 1..96", n);
    EVC_REQUIRE(in != out && in != tmp && out != tmp && three_quarter != out && three_quarter != tmp &&
                    three_quarter != in,
                "evc_four_index_transform: buffers must not alias");
    hipStream_t st = as_stream(stream);
    auto qt = [&](const double *src, double *dst) {
        return launch_quarter_transform(src, 0, C, 0, c_transposed, n, dst, 0, 1, st);
    };
    // in -> out -> tmp -> (three_quarter | out) -> out ; the third result must survive in
    // `three_quarter` when requested, otherwise ping-pong between out and tmp.
    int rc;
    if ((rc = qt(in, out))) return rc;
    if ((rc = qt(out, tmp))) return rc;
    double *third = three_quarter ? three_quarter : out;
    if ((rc = qt(tmp, third))) return rc;
    if (three_quarter) return qt(third, out);
    if ((rc = qt(third, tmp))) return rc;
    // result sits in tmp: copy back (device-to-device, same stream)
    hipError_t e = hipMemcpyAsync(out, tmp, sizeof(double) * (size_t)n * n * n * n, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
        set_error("evc_four_index_transform: copy failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}
