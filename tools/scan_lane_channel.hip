// Standalone probe: the selective scan's emitting pass in the OTHER lane mapping - lane = channel, the 16 states of the
// channel in registers, Bm_t / Cm_t as wave-uniform values - timed beside the library's scan_emit_kernel (lane = (channel,
// state), csrc/mamba.hip, included below) on the same chunked problem: B = 12, L = 962, chunks of SCAN_CHUNK positions
// starting from the same chunk-start states, D = 128 .. 1024.  Both kernels read u, delta_raw, z, Bm, Cm once and write y
// once; results are compared element by element.  DESIGN 3.9 quotes the table this prints.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 tools/scan_lane_channel.hip -o tools/scan_lane_channel.bin
#include "../deepsense6g_tii_amd/csrc/mamba.hip"

#include <cmath>
#include <cstdlib>
#include <vector>

int g_ds6g_bf16 = 0;   // common.h declares them; the probe links no other library source
thread_local const uint64_t* g_ds6g_salt = nullptr;

namespace {

// one wave = 64 channels of one chunk; no LDS, no cross-lane traffic
__global__ __launch_bounds__(64) void scan_emit_lane_channel_kernel(const ScanP p) {
    const int c = blockIdx.y, b = blockIdx.z;
    const int d = blockIdx.x * 64 + threadIdx.x;
    const int s0 = c * SCAN_CHUNK;
    const int len = min(SCAN_CHUNK, p.L - s0);
    const size_t rowbase = (size_t)b * p.L;
    const size_t chunk_id = (size_t)b * p.nc + c;
    float A2[NS], h[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) {
        A2[n] = -expf(p.A_log[d * NS + n]) * LOG2E;
        h[n] = c > 0 ? p.hin[(chunk_id * p.D + d) * NS + n] : 0.f;
    }
    const float Dd = p.Dp[d], bias = p.dt_bias[d];
    for (int s = 0; s < len; ++s) {
        const size_t row = rowbase + (p.rev ? p.L - 1 - (s0 + s) : s0 + s);
        const float dt = softplus_(p.raw[row * p.ld_raw + d] + bias);
        const float uu = p.u[row * p.ld_u + d], zz = p.z[row * p.ld_z + d];
        const float* __restrict__ Bt = p.Bm + row * p.ld_b;   // wave-uniform addresses: scalar loads
        const float* __restrict__ Ct = p.Cm + row * p.ld_c;
        const float du = dt * uu;
        float acc = Dd * uu;
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            h[n] = fmaf(exp2f(dt * A2[n]), h[n], du * Bt[n]);
            acc = fmaf(h[n], Ct[n], acc);
        }
        p.y[row * p.ld_y + d] = acc * zz * sigmoid_(zz);
    }
}

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

float* dev_random(size_t n, float scale, unsigned seed) {
    std::vector<float> h(n);
    srand(seed);
    for (auto& v : h) v = scale * ((float)rand() / (float)RAND_MAX * 2.f - 1.f);
    float* d;
    HIP_OK(hipMalloc(&d, n * sizeof(float)));
    HIP_OK(hipMemcpy(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    return d;
}

template <typename F>
float time_us(F launch, int iters) {
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    for (int i = 0; i < 5; ++i) launch();
    HIP_OK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        HIP_OK(hipEventRecord(e0));
        for (int i = 0; i < iters; ++i) launch();
        HIP_OK(hipEventRecord(e1));
        HIP_OK(hipEventSynchronize(e1));
        float ms; HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        best = fminf(best, ms * 1e3f / iters);
    }
    return best;
}

}  // namespace

int main() {
    const int B = 12, L = 962;
    printf("scan emitting pass, B = %d, L = %d, chunk %d: lane = (channel, state) [library] vs lane = channel [probe]\n", B, L,
           SCAN_CHUNK);
    printf("%8s %22s %18s %14s\n", "d_inner", "lane=(chan,state) us", "lane=channel us", "max |diff|");
    for (int D : {128, 256, 512, 1024}) {
        const size_t M = (size_t)B * L;
        const int nc = (L + SCAN_CHUNK - 1) / SCAN_CHUNK;
        ScanP p{};
        p.u = dev_random(M * D, 1.f, 1); p.raw = dev_random(M * D, 1.f, 2); p.z = dev_random(M * D, 1.f, 3);
        p.Bm = dev_random(M * 16, 1.f, 4); p.Cm = dev_random(M * 16, 1.f, 5);
        p.dt_bias = dev_random(D, 1.f, 6); p.A_log = dev_random((size_t)D * 16, 1.f, 7); p.Dp = dev_random(D, 1.f, 8);
        p.hin = dev_random((size_t)B * nc * D * 16, 1.f, 9);
        p.ld_u = p.ld_raw = p.ld_z = p.ld_y = D; p.ld_b = p.ld_c = 16;
        p.B = B; p.L = L; p.D = D; p.nc = nc; p.rev = 0;
        float *y0, *y1;
        HIP_OK(hipMalloc(&y0, M * D * sizeof(float))); HIP_OK(hipMalloc(&y1, M * D * sizeof(float)));
        ScanP p0 = p, p1 = p;
        p0.y = y0; p1.y = y1;
        const float t0 = time_us([&] { hipLaunchKernelGGL(scan_emit_kernel, dim3(D / CPB, nc, B), dim3(256), 0, 0, p0); }, 20);
        const float t1 = time_us([&] { hipLaunchKernelGGL(scan_emit_lane_channel_kernel, dim3(D / 64, nc, B), dim3(64), 0, 0, p1); }, 20);
        HIP_OK(hipGetLastError());
        std::vector<float> a(M * D), c(M * D);
        HIP_OK(hipMemcpy(a.data(), y0, M * D * sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(c.data(), y1, M * D * sizeof(float), hipMemcpyDeviceToHost));
        float md = 0.f;
        for (size_t i = 0; i < M * D; ++i) md = fmaxf(md, fabsf(a[i] - c[i]));
        printf("%8d %22.1f %18.1f %14.3e\n", D, t0, t1, md);
        for (const float* q : {p.u, p.raw, p.z, p.Bm, p.Cm, p.dt_bias, p.A_log, p.Dp}) HIP_OK(hipFree((void*)q));
        HIP_OK(hipFree(p.hin)); HIP_OK(hipFree(y0)); HIP_OK(hipFree(y1));
    }
    return 0;
}
