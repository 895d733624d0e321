// Standalone kernel micro-benchmark (development tool, not shipped): times the product kernels
// and experimental variants on B pairs of S^3 random volumes with hipEvents.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/kbench.hip -o build/kbench && build/kbench 8 256
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../torchregister_amd/csrc/affine.hip"
#include "../torchregister_amd/csrc/affine_finalize.hip"   // the loss / backward finalise launchers affine.hip's entry points call

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } } while (0)

// E1: streaming skeleton — aligned read of moving + target, 5 moments, same block geometry
__global__ __launch_bounds__(256) void skel_kernel(trx_volumes vol, trx::AffineGeom g, float *partials)
{
    const int b = blockIdx.y;
    int id = blockIdx.x;
    const int xs = id % g.nxseg; id /= g.nxseg;
    const int yc = id % g.nychunk;
    const int z = id / g.nychunk;
    const int tid = threadIdx.x;
    const int lx = tid & (g.TX - 1), ly = tid >> g.logTX;
    const int x = xs * g.TX + lx;
    const int H = vol.H, W = vol.W;
    const float *mov = vol.moving + (size_t)b * vol.moving_stride;
    const float *tgt = vol.target + (size_t)b * vol.target_stride;
    float m[5] = {0, 0, 0, 0, 0};
    if (x < W) {
        const int y0 = yc * g.TY * g.RPT + ly;
        for (int j = 0; j < g.RPT; j++) {
            const int y = y0 + j * g.TY;
            if (y >= H) break;
            const size_t vox = ((size_t)z * H + y) * W + x;
            const float yv = tgt[vox], w = mov[vox];
            m[0] += yv; m[1] += w; m[2] = fmaf(yv, yv, m[2]); m[3] = fmaf(w, w, m[3]); m[4] = fmaf(yv, w, m[4]);
        }
    }
    trx::block_reduce_store<5>(m, partials + ((size_t)b * g.nblk + blockIdx.x) * 5);
}

// E1b: float4 grid-stride skeleton (best-case streaming read of both volumes)
__global__ __launch_bounds__(256) void skel4_kernel(const float4 *a, const float4 *b, size_t n4, float *partials)
{
    float m[5] = {0, 0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float4 u = a[i], v = b[i];
        m[0] += u.x + u.y + u.z + u.w; m[1] += v.x + v.y + v.z + v.w;
        m[2] += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w; m[3] += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        m[4] += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
    }
    trx::block_reduce_store<5>(m, partials + (size_t)blockIdx.x * 5);
}

template <typename F>
static float time_it(F f, int reps)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    f(); f();
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    for (int i = 0; i < reps; i++) f();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1000.f / reps;
}

int main(int argc, char **argv)
{
    setvbuf(stdout, nullptr, _IONBF, 0);
    int B = argc > 1 ? atoi(argv[1]) : 8, S = argc > 2 ? atoi(argv[2]) : 256;
    int tb = argc > 3 ? atoi(argv[3]) : trx::kTargetBlocks;
    const int Wx = argc > 4 ? atoi(argv[4]) : S;   // optional row length (volume S x S x Wx) to probe pitch effects
    size_t nvox = (size_t)S * S * Wx, n = nvox * B;
    std::vector<float> h(n);
    srand(1);
    for (size_t i = 0; i < n; i++) h[i] = (float)rand() / RAND_MAX;
    float *mov, *tgt, *theta, *partials;
    CK(hipMalloc(&mov, n * 4)); CK(hipMalloc(&tgt, n * 4));
    CK(hipMemcpy(mov, h.data(), n * 4, hipMemcpyHostToDevice));
    for (size_t i = 0; i < n; i++) h[i] = (float)rand() / RAND_MAX;
    CK(hipMemcpy(tgt, h.data(), n * 4, hipMemcpyHostToDevice));
    std::vector<float> th(B * 12);
    const float t0[12] = {0.95f, -0.1f, 0.02f, 0.05f, 0.1f, 0.97f, 0.0f, -0.03f, 0.0f, 0.03f, 1.02f, 0.02f};
    for (int b = 0; b < B; b++) for (int i = 0; i < 12; i++) th[b * 12 + i] = t0[i];
    CK(hipMalloc(&theta, B * 12 * 4));
    CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
    float *tab;
    CK(hipMalloc(&tab, (2 * S + Wx) * 4));
    hipLaunchKernelGGL(trx::fill_tables_kernel, dim3((std::max(S, Wx) + 255) / 256), dim3(256), 0, 0, tab, Wx, S, S);
    trx_volumes vol = {mov, tgt, nvox, nvox, 3, B, S, S, Wx, tab, tab + Wx, tab + Wx + S};
    trx::AffineGeom g = trx::affine_geom(vol, tb);
    CK(hipMalloc(&partials, (size_t)B * (g.nblk + 4096) * 41 * 4 + 4096));
    printf("B=%d S=%d W=%d geom TX=%d TY=%d RPT=%d nblk=%d\n", B, S, Wx, g.TX, g.TY, g.RPT, g.nblk);
    dim3 grid(g.nblk, B), block(256);
    const double alg = 8.0 * nvox;  // bytes per pair-iteration
    auto rep = [&](const char *name, float us) {
        printf("%-28s %9.1f us/launch  %7.2f us/pair  %6.2f TB/s alg\n", name, us, us / B, alg * B / us / 1e6);
    };
    rep("skel (dword, same geom)", time_it([&] { hipLaunchKernelGGL(skel_kernel, grid, block, 0, 0, vol, g, partials); }, 20));
    rep("skel4 (float4 grid-stride)", time_it([&] { hipLaunchKernelGGL(skel4_kernel, dim3(4096), block, 0, 0, (const float4 *)mov, (const float4 *)tgt, n / 4, partials); }, 20));
    rep("accum MODE1 (moments)", time_it([&] { hipLaunchKernelGGL((trx::affine_accum_kernel<3, 1>), grid, block, 0, 0, vol, theta, g, 1, (size_t)0, partials); }, 20));
    rep("accum MODE0 (full F1)", time_it([&] { hipLaunchKernelGGL((trx::affine_accum_kernel<3, 0>), grid, block, 0, 0, vol, theta, g, 1, (size_t)0, partials); }, 20));
    trx::TileGeom tgm = trx::tile_geom(vol);
    printf("tile geom: %d x %d x %d tiles, %d blocks/pair\n", tgm.ntx, tgm.nty, tgm.ntz, tgm.blocks_per_pair);
    dim3 tgrid(tgm.blocks_per_pair, B);
    rep("tile MODE1 (moments)", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<1>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 20));
    rep("tile MODE0 (full F1)", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<0>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 20));
    {   // the dual kernel in GeomA mode: the cost of the surplus (empty) blocks
        const trx::TileGeom ta = trx::tile_geom<trx::GeomA>(vol), tr = trx::tile_geom<trx::GeomR>(vol);
        const int gx = ta.blocks_per_pair > tr.blocks_per_pair ? ta.blocks_per_pair : tr.blocks_per_pair;
        rep("dual MODE0 (GeomA chosen)", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_dual_kernel<0>), dim3(gx, B), dim3(512), 0, 0, vol, theta, ta, tr, 1, partials); }, 20));
    }
#if TRX_TIMING
    {
        std::vector<unsigned long long> tmv(4 * 8192);
        CK(hipMemcpyFromSymbol(tmv.data(), HIP_SYMBOL(trx::trx_timing), tmv.size() * 8));
        const size_t nb = std::min<size_t>(8192, (size_t)tgrid.x * tgrid.y);
        double a[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < nb; i++) for (int k = 0; k < 4; k++) a[k] += (double)tmv[i * 4 + k];
        const double tiles = (double)tgm.nty / tgm.ysplit;
        printf("  timing per tile (s_memtime ticks, wave 0 avg over %zu blocks): issue+wait %.0f  barrier1 %.0f  gather %.0f  barrier2 %.0f\n",
               nb, a[0] / nb / tiles, a[1] / nb / tiles, a[2] / nb / tiles, a[3] / nb / tiles);
    }
#endif
    // identity theta (all samples on voxel centres)
    const float id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int b = 0; b < B; b++) for (int i = 0; i < 12; i++) th[b * 12 + i] = id[i];
    CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
    rep("accum MODE0 identity", time_it([&] { hipLaunchKernelGGL((trx::affine_accum_kernel<3, 0>), grid, block, 0, 0, vol, theta, g, 1, (size_t)0, partials); }, 20));
    {   // large rotation (0.5 rad about z): no tile fits the LDS box -> in-kernel global-gather fallback
        const float rt[12] = {0.8776f, -0.4794f, 0.f, 0.02f, 0.4794f, 0.8776f, 0.f, -0.01f, 0.f, 0.f, 1.f, 0.f};
        for (int b = 0; b < B; b++) for (int i = 0; i < 12; i++) th[b * 12 + i] = rt[i];
        CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
        rep("tile MODE0 rot 0.5 (fallback)", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<0>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 10));
        {   // the dual kernel picks GeomR for this theta
            const trx::TileGeom ta = trx::tile_geom<trx::GeomA>(vol), tr = trx::tile_geom<trx::GeomR>(vol);
            const int gx = ta.blocks_per_pair > tr.blocks_per_pair ? ta.blocks_per_pair : tr.blocks_per_pair;
            rep("dual MODE0 rot 0.5 (GeomR)", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_dual_kernel<0>), dim3(gx, B), dim3(512), 0, 0, vol, theta, ta, tr, 1, partials); }, 10));
        }
        {   // a general rotation (Rz(0.6) Ry(0.8) Rx(0.7), what the reference's random rigid init looks like)
            const double a = 0.8, bz = 0.6, c = 0.7;
            const double Ry[9] = {cos(a), 0, sin(a), 0, 1, 0, -sin(a), 0, cos(a)}, Rz[9] = {cos(bz), -sin(bz), 0, sin(bz), cos(bz), 0, 0, 0, 1},
                         Rx[9] = {1, 0, 0, 0, cos(c), -sin(c), 0, sin(c), cos(c)};
            double T[9], R[9];
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { T[i * 3 + j] = 0; for (int k = 0; k < 3; k++) T[i * 3 + j] += Rz[i * 3 + k] * Ry[k * 3 + j]; }
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { R[i * 3 + j] = 0; for (int k = 0; k < 3; k++) R[i * 3 + j] += T[i * 3 + k] * Rx[k * 3 + j]; }
            for (int b = 0; b < B; b++) for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) th[b * 12 + i * 4 + j] = (float)R[i * 3 + j]; th[b * 12 + i * 4 + 3] = 0.01f * (i + 1); }
            CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
            const trx::TileGeom ta = trx::tile_geom<trx::GeomA>(vol), tr = trx::tile_geom<trx::GeomR>(vol);
            const int gx = ta.blocks_per_pair > tr.blocks_per_pair ? ta.blocks_per_pair : tr.blocks_per_pair;
            rep("dual MODE0 rot .8/.6/.7", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_dual_kernel<0>), dim3(gx, B), dim3(512), 0, 0, vol, theta, ta, tr, 1, partials); }, 10));
            rep("tile MODE0 rot .8/.6/.7", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<0>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 10));
            {   // a moderate general rotation (0.4 rad about every axis) and 0.3 rad about z: the single-geometry kernel only (GeomA)
                for (int which = 0; which < 2; which++) {
                    const double a2 = which ? 0.0 : 0.4, b2 = which ? 0.3 : 0.4, c2 = which ? 0.0 : 0.4;
                    const double Ry2[9] = {cos(a2), 0, sin(a2), 0, 1, 0, -sin(a2), 0, cos(a2)}, Rz2[9] = {cos(b2), -sin(b2), 0, sin(b2), cos(b2), 0, 0, 0, 1},
                                 Rx2[9] = {1, 0, 0, 0, cos(c2), -sin(c2), 0, sin(c2), cos(c2)};
                    double T2[9], R2[9];
                    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { T2[i * 3 + j] = 0; for (int k = 0; k < 3; k++) T2[i * 3 + j] += Rz2[i * 3 + k] * Ry2[k * 3 + j]; }
                    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { R2[i * 3 + j] = 0; for (int k = 0; k < 3; k++) R2[i * 3 + j] += T2[i * 3 + k] * Rx2[k * 3 + j]; }
                    for (int b = 0; b < B; b++) for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) th[b * 12 + i * 4 + j] = (float)R2[i * 3 + j]; th[b * 12 + i * 4 + 3] = 0.01f * (i + 1); }
                    CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
                    rep(which ? "tile MODE0 rot z 0.3" : "tile MODE0 rot .4/.4/.4", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<0>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 10));
                }
            }
            for (int b = 0; b < B; b++) for (int i = 0; i < 12; i++) th[b * 12 + i] = rt[i];
            CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
        }
        rep("accum MODE0 rot 0.5 (gather kernel)", time_it([&] { hipLaunchKernelGGL((trx::affine_accum_kernel<3, 0>), grid, block, 0, 0, vol, theta, g, 1, (size_t)0, partials); }, 10));
        for (int b = 0; b < B; b++) for (int i = 0; i < 12; i++) th[b * 12 + i] = id[i];
        CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
    }
    rep("tile MODE0 identity (before)", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<0>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 20));
    {
        const trx::TileGeom ta = trx::tile_geom<trx::GeomA>(vol), tr = trx::tile_geom<trx::GeomR>(vol);
        const int gx = ta.blocks_per_pair > tr.blocks_per_pair ? ta.blocks_per_pair : tr.blocks_per_pair;
        rep("dual MODE0 identity", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_dual_kernel<0>), dim3(gx, B), dim3(512), 0, 0, vol, theta, ta, tr, 1, partials); }, 20));
    }
    rep("tile MODE0 identity", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<0>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 20));
    {   // what bench.py's run looks like after its 125 Adam iterations: |theta - I| ~ 0.0125, plus a shift
        const float sm[12] = {1.011f, -0.012f, 0.009f, 0.02f, 0.0125f, 0.992f, -0.007f, -0.015f, -0.01f, 0.011f, 1.006f, 0.01f};
        for (int b = 0; b < B; b++) for (int i = 0; i < 12; i++) th[b * 12 + i] = sm[i];
        CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
        rep("tile MODE0 |theta-I| 0.0125", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<0>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 20));
        const float s3[12] = {1.02f, -0.03f, 0.015f, 0.03f, 0.03f, 0.985f, -0.012f, -0.02f, -0.015f, 0.02f, 1.01f, 0.015f};
        for (int b = 0; b < B; b++) for (int i = 0; i < 12; i++) th[b * 12 + i] = s3[i];
        CK(hipMemcpy(theta, th.data(), B * 12 * 4, hipMemcpyHostToDevice));
        rep("tile MODE0 rot 0.03", time_it([&] { hipLaunchKernelGGL((trx::affine_tile_kernel<0>), tgrid, dim3(trx::kTileThreads), 0, 0, vol, theta, tgm, 1, partials); }, 20));
    }
    return 0;
}
