// Stand-alone check of the host-side argument checking of csrc/chain.hip (trx_transform_points, trx_affine_then_flow_resample): every refusal path is
// called with pointers that are not mapped, so nothing may reach a device - a CPU-only program, meant to be built with the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -c torchregister_amd/csrc/chain.hip -o chain_asan.o
//   hipcc -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -c tools/chain_host_check.cpp -o chain_host_check.o
//   hipcc -fsanitize=address,undefined chain_asan.o chain_host_check.o -o chain_host_check && ./chain_host_check
// It prints the number of refusals checked and exits 0, or names the first call whose status is not the documented one and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../include/trx.h"

namespace {

int checked = 0;

void expect(int got, int want, const char *what)
{
    checked++;
    if (got != want) {
        std::fprintf(stderr, "%s: status %d, expected %d\n", what, got, want);
        std::exit(1);
    }
}

const float *fp(uintptr_t a) { return reinterpret_cast<const float *>(a); }
float *fpw(uintptr_t a) { return reinterpret_cast<float *>(a); }

constexpr uintptr_t MB = 1u << 20;

struct Points {
    uintptr_t points = MB, out = 2 * MB, theta = 3 * MB, flow = 4 * MB;
    int ndim = 3, B = 1, P = 10, chain = 0, padding = 1;
    int from[3] = {5, 6, 7}, to[3] = {5, 6, 7};
    bool has_from = true, has_to = true;
    int call() const
    {
        return trx_transform_points(fp(points), fpw(out), ndim, B, P, fp(theta), fp(flow), has_from ? from : nullptr, has_to ? to : nullptr, chain, padding, nullptr);
    }
};

struct Image {
    uintptr_t src = MB, out = 8 * MB, theta = 3 * MB, flow = 4 * MB;
    size_t stride = 420;
    int ndim = 3, B = 1, channels = 2, order = 1, padding = 1;
    int ssize[3] = {5, 6, 7}, osize[3] = {4, 5, 6};
    bool has_ssize = true, has_osize = true;
    int call() const
    {
        return trx_affine_then_flow_resample(fp(src), stride, has_ssize ? ssize : nullptr, fp(theta), fp(flow), ndim, B, channels, has_osize ? osize : nullptr, order,
                                             padding, fpw(out), nullptr);
    }
};

template <class T, class F> int with(F &&change)
{
    T t;
    change(t);
    return t.call();
}

}  // namespace

int main()
{
    const int ARG = TRX_ERR_ARG, NDIM = TRX_ERR_NDIM;
    // NULLs
    expect(with<Points>([](Points &p) { p.points = 0; }), ARG, "points NULL");
    expect(with<Points>([](Points &p) { p.out = 0; }), ARG, "points: out NULL");
    expect(with<Points>([](Points &p) { p.theta = p.flow = 0; }), ARG, "points: theta and flow NULL");
    expect(with<Points>([](Points &p) { p.has_from = false; }), ARG, "points: from_size NULL");
    expect(with<Points>([](Points &p) { p.has_to = false; }), ARG, "points: to_size NULL with theta");
    expect(with<Points>([](Points &p) { p.has_to = false; p.theta = 0; p.chain = 1; }), ARG, "points: to_size NULL in chain 1");
    expect(with<Image>([](Image &i) { i.src = 0; }), ARG, "image: src NULL");
    expect(with<Image>([](Image &i) { i.out = 0; }), ARG, "image: out NULL");
    expect(with<Image>([](Image &i) { i.theta = i.flow = 0; }), ARG, "image: theta and flow NULL");
    expect(with<Image>([](Image &i) { i.has_ssize = false; }), ARG, "image: src_size NULL");
    expect(with<Image>([](Image &i) { i.has_osize = false; }), ARG, "image: out_size NULL");
    // theta NULL with unequal lattices
    expect(with<Points>([](Points &p) { p.theta = 0; p.chain = 1; p.to[2] = 8; }), ARG, "points: theta NULL, unequal lattices, chain 1");
    expect(with<Image>([](Image &i) { i.theta = 0; }), ARG, "image: theta NULL, unequal lattices");
    // ndim
    for (int bad : {0, 1, 4, -3}) {
        expect(with<Points>([&](Points &p) { p.ndim = bad; }), NDIM, "points: ndim");
        expect(with<Image>([&](Image &i) { i.ndim = bad; }), NDIM, "image: ndim");
    }
    expect(with<Points>([](Points &p) { p.ndim = 5; p.points = 0; p.chain = 9; }), NDIM, "points: ndim wins");
    expect(with<Image>([](Image &i) { i.ndim = 5; i.src = 0; i.order = 7; }), NDIM, "image: ndim wins");
    expect(with<Points>([](Points &p) { p.ndim = 2; }), NDIM, "points: 2-D with D != 1");
    expect(with<Points>([](Points &p) { p.ndim = 2; p.from[0] = 1; }), NDIM, "points: 2-D with to D != 1");
    expect(with<Image>([](Image &i) { i.ndim = 2; }), NDIM, "image: 2-D with D != 1");
    expect(with<Image>([](Image &i) { i.ndim = 2; i.ssize[0] = 1; i.stride = 84; }), NDIM, "image: 2-D with out D != 1");
    // sizes
    const int sizes[4][3] = {{0, 6, 7}, {5, -1, 7}, {5, 6, 0}, {2048, 1024, 1024}};
    for (const auto &s : sizes) {
        expect(with<Points>([&](Points &p) { for (int k = 0; k < 3; k++) p.from[k] = s[k]; }), ARG, "points: from_size");
        expect(with<Points>([&](Points &p) { for (int k = 0; k < 3; k++) p.to[k] = s[k]; }), ARG, "points: to_size");
        expect(with<Image>([&](Image &i) { for (int k = 0; k < 3; k++) i.osize[k] = s[k]; }), ARG, "image: out_size");
        expect(with<Image>([&](Image &i) { for (int k = 0; k < 3; k++) i.ssize[k] = s[k]; i.stride = (size_t)1 << 32; }), ARG, "image: src_size");
    }
    for (int bad : {0, -1, 65536}) {
        expect(with<Points>([&](Points &p) { p.B = bad; }), ARG, "points: B");
        expect(with<Image>([&](Image &i) { i.B = bad; }), ARG, "image: B");
    }
    for (int bad : {0, -5}) {
        expect(with<Points>([&](Points &p) { p.P = bad; }), ARG, "points: P");
        expect(with<Image>([&](Image &i) { i.channels = bad; }), ARG, "image: channels");
    }
    expect(with<Image>([](Image &i) { i.stride = 419; }), ARG, "image: src_stride below a pair's channels");
    // enums
    for (int bad : {-1, 2, 3}) {
        expect(with<Points>([&](Points &p) { p.padding = bad; }), ARG, "points: padding");
        expect(with<Points>([&](Points &p) { p.chain = bad; }), ARG, "points: chain");
        expect(with<Image>([&](Image &i) { i.padding = bad; }), ARG, "image: padding");
    }
    for (int bad : {-1, 2, 4, 5}) expect(with<Image>([&](Image &i) { i.order = bad; }), ARG, "image: order");
    // overlap
    expect(with<Image>([](Image &i) { i.out = MB; }), ARG, "image: out == src");
    expect(with<Image>([](Image &i) { i.out = MB + 16; }), ARG, "image: out inside src");
    expect(with<Image>([](Image &i) { i.out = MB - 956; }), ARG, "image: out's last float is src's first");
    expect(with<Image>([](Image &i) { i.out = 4 * MB; }), ARG, "image: out == flow");
    expect(with<Image>([](Image &i) { i.out = 4 * MB + 2516; }), ARG, "image: out on flow's last float");
    expect(with<Image>([](Image &i) { i.B = 65535; i.stride = (size_t)1 << 40; i.out = MB + ((uintptr_t)1 << 42); }), ARG, "image: out inside a strided batch");
    expect(with<Points>([](Points &p) { p.out = MB + 4; }), ARG, "points: out overlaps points without being points");
    expect(with<Points>([](Points &p) { p.out = 4 * MB; }), ARG, "points: out == flow");
    expect(with<Points>([](Points &p) { p.out = 4 * MB + 2516; }), ARG, "points: out on flow's last float");
    std::printf("chain host check: %d refusals, all with the documented status\n", checked);
    return 0;
}
