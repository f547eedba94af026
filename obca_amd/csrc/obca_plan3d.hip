// obca_plan3d.hip -- libobca_plan3d.so: the C ABI of include/obca_plan3d.h around the kernel of obca_plan3d.h.  A library of its own (the product library
// libobca_hip.so and the host planner libobca_plan.so neither contain nor link it).  One call = one upload of the instances' records, one kernel (a workgroup per
// instance, the grid in its LDS), one download; the buffers live with the context and only grow.  No CPU fallback: without a device there is no context.
// Build: hipcc (obca_amd/buildflags.py HIPCC) -o libobca_plan3d.so obca_plan3d.hip   (tools/build.sh, __graft_entry__.build()).
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include <vector>
#include "obca_plan3d.h"
#include "../../include/obca_hip.h"

static_assert(OBCA_PLAN3D_NMAX == OBCA_QUAD_NMAX, "the warm start's horizon limit is the quadcopter solve's");
static_assert((OBCA_PLAN3D_MAXCELLS + 4) * sizeof(float) <= 160 * 1024, "the field and its control words must fit the LDS of one workgroup");

using namespace obca;

__global__ __launch_bounds__(PL3_NT) void obca_plan3d_kernel(const double *in, int nBox, double clear, double room0, double room1, double room2, double res, int nx, int ny, int nz,
                                                             double *paths, int cap, int *counts, int *sweeps, int N, double *xws) {
    extern __shared__ float pl3_lds[];
    pl3::Grid G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.ncell = nx * ny * nz; G.nBox = nBox; G.res = res; G.clear = clear; G.room[0] = room0; G.room[1] = room1; G.room[2] = room2; G.boxes = nullptr;
    const size_t i = blockIdx.x;
    pl3::plan_instance(in + i * PL3_IN_STRIDE(nBox), G, pl3_lds, paths + i * (size_t)cap * 3, cap, counts + i, sweeps + i, N, xws ? xws + i * (size_t)(N + 1) * 12 : nullptr);
}

namespace {

thread_local std::string g_create_err;

struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double *d_in = nullptr, *d_paths = nullptr, *d_xws = nullptr; int *d_counts = nullptr;      // d_counts: counts, then sweeps
    size_t n_in = 0, n_paths = 0, n_xws = 0, n_counts = 0;
    int lds_set = 0;
    float ms = 0.f;
    std::string err;
    std::vector<double> h_in; std::vector<int> h_counts;
};

#define PL3_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { c->err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } } while (0)

template <class T> int grow(Ctx *c, T *&p, size_t &have, size_t want) {
    if (want <= have) return 0;
    if (p) { PL3_HIP(hipFree(p)); p = nullptr; have = 0; }
    PL3_HIP(hipMalloc((void **)&p, want * sizeof(T)));
    have = want;
    return 0;
}

// the common path of both entry points.  pts: B x pstride (first three doubles the position); paths_out (B x cap x 3) or xws_out (B x (N+1) x 12)
int run(Ctx *c, const char *who, int B, int N, const double *starts, const double *goals, int pstride, int nBox, const double *boxes, double clear, const double *room, double res,
        double *paths_out, int cap, int *counts, int *sweeps, double *xws_out) {
    if (!counts || (!paths_out && !xws_out)) { c->err = std::string(who) + ": need non-NULL output arrays"; return -1; }
    int dims[3];
    const char *bad = pl3::check_args(B, starts, goals, pstride, nBox, boxes, clear, room, res, cap, N, xws_out != nullptr, dims);
    if (bad) { c->err = std::string(who) + ": " + bad; return -1; }
    PL3_HIP(hipSetDevice(c->device));
    const int stride = PL3_IN_STRIDE(nBox), ncell = dims[0] * dims[1] * dims[2];
    c->h_in.resize((size_t)B * stride);
    for (int i = 0; i < B; i++) {
        double *r = c->h_in.data() + (size_t)i * stride;
        memcpy(r, starts + (size_t)i * pstride, 3 * sizeof(double)); memcpy(r + 3, goals + (size_t)i * pstride, 3 * sizeof(double));
        if (nBox) memcpy(r + 6, boxes + (size_t)i * nBox * 6, (size_t)nBox * 6 * sizeof(double));
    }
    const size_t npaths = (size_t)B * cap * 3, nxws = xws_out ? (size_t)B * (N + 1) * 12 : 0;
    if (grow(c, c->d_in, c->n_in, c->h_in.size()) || grow(c, c->d_paths, c->n_paths, npaths) || grow(c, c->d_counts, c->n_counts, (size_t)2 * B) || (nxws && grow(c, c->d_xws, c->n_xws, nxws))) return -2;
    const int lds = (ncell + 4) * (int)sizeof(float);
    if (lds > c->lds_set) { PL3_HIP(hipFuncSetAttribute((const void *)obca_plan3d_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds)); c->lds_set = lds; }
    PL3_HIP(hipMemcpyAsync(c->d_in, c->h_in.data(), c->h_in.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PL3_HIP(hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(obca_plan3d_kernel, dim3(B), dim3(PL3_NT), lds, c->stream, c->d_in, nBox, clear, room[0], room[1], room[2], res, dims[0], dims[1], dims[2],
                       c->d_paths, cap, c->d_counts, c->d_counts + B, xws_out ? N : 0, xws_out ? c->d_xws : nullptr);
    PL3_HIP(hipGetLastError());
    PL3_HIP(hipEventRecord(c->ev1, c->stream));
    c->h_counts.resize((size_t)2 * B);
    PL3_HIP(hipMemcpyAsync(c->h_counts.data(), c->d_counts, (size_t)2 * B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (paths_out) PL3_HIP(hipMemcpyAsync(paths_out, c->d_paths, npaths * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (xws_out) PL3_HIP(hipMemcpyAsync(xws_out, c->d_xws, nxws * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PL3_HIP(hipStreamSynchronize(c->stream));
    PL3_HIP(hipEventElapsedTime(&c->ms, c->ev0, c->ev1));
    memcpy(counts, c->h_counts.data(), (size_t)B * sizeof(int));
    if (sweeps) memcpy(sweeps, c->h_counts.data() + B, (size_t)B * sizeof(int));
    return 0;
}

}  // namespace

extern "C" {

int obca_plan3d_create(int device, void **ctx) {
    if (!ctx) { g_create_err = "obca_plan3d_create: ctx is NULL"; return -1; }
    *ctx = nullptr;
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) { g_create_err = std::string("obca_plan3d_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") + "); there is no CPU fallback"; return -2; }
    if (device < 0 || device >= ndev) { g_create_err = "obca_plan3d_create: no such device"; return -2; }
    Ctx *c = new Ctx; c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        g_create_err = "obca_plan3d_create: cannot create the stream and events on the device"; delete c; return -2;
    }
    *ctx = c;
    return 0;
}

int obca_plan3d_destroy(void *ctx) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return -1;
    (void)hipSetDevice(c->device);
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->d_paths) (void)hipFree(c->d_paths);
    if (c->d_xws) (void)hipFree(c->d_xws);
    if (c->d_counts) (void)hipFree(c->d_counts);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

const char *obca_plan3d_last_error(void *ctx) { return ctx ? ((Ctx *)ctx)->err.c_str() : g_create_err.c_str(); }

int obca_plan3d_paths_batch(void *ctx, int B, const double *starts, const double *goals, int nBox, const double *boxes, double clear, const double room[3],
                            double res, double *paths, int cap, int *counts, int *sweeps) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return -1;
    if (!paths) { c->err = "obca_plan3d_paths_batch: paths is NULL"; return -1; }
    return run(c, "obca_plan3d_paths_batch", B, 0, starts, goals, 3, nBox, boxes, clear, room, res, paths, cap, counts, sweeps, nullptr);
}

int obca_plan3d_warm_start_batch(void *ctx, int B, int N, const double *x0, const double *xF, int nBox, const double *boxes, double clear, const double room[3],
                                 double res, double *xWS, int *counts) {
    Ctx *c = (Ctx *)ctx;
    if (!c) return -1;
    if (!xWS) { c->err = "obca_plan3d_warm_start_batch: xWS is NULL"; return -1; }
    return run(c, "obca_plan3d_warm_start_batch", B, N, x0, xF, 12, nBox, boxes, clear, room, res, nullptr, OBCA_PLAN3D_WS_CAP, counts, nullptr, xWS);
}

int obca_plan3d_kernel_ms(void *ctx, float *ms) {
    Ctx *c = (Ctx *)ctx;
    if (!c || !ms) return -1;
    *ms = c->ms;
    return 0;
}

}  // extern "C"
