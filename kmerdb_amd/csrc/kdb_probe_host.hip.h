// kdb_probe_host.hip.h -- the memory system's ceilings for the kernels' access patterns (diagnostic; bench.py): the table of patterns
// (kernels: kdb_probe.hip.h) and the kdb_hbm_pattern_* calls that time them.  No engine.
#pragma once
#include "kdb_hostutil.hip.h"
#include "kdb_probe.hip.h"

namespace {
struct ProbePattern { const char *name; void (*launch)(const uint8_t *, uint64_t, uint8_t *, uint64_t, uint32_t, uint32_t *, hipStream_t); uint32_t read_bytes, write_bytes; };
template <int RM, int WM, int NR, int NW>
void probe_launch(const uint8_t *src, uint64_t sb, uint8_t *dst, uint64_t db, uint32_t steps, uint32_t *sink, hipStream_t st)
{
    hipLaunchKernelGGL((kdbprobe::pattern<RM, WM, NR, NW>), dim3(512), dim3(512), 0, st, src, sb, dst, db, steps, sink);
}
using namespace kdbprobe;
#define KDB_PROBE(name, RM, WM, NR, NW) {name, probe_launch<RM, WM, NR, NW>, (uint32_t)(NR * (RM == R_PAGES15 ? 1536 : RM ? 1024 : 0)), (uint32_t)(NW * (WM ? 1024 : 0))}
const ProbePattern PROBES[] = {
    KDB_PROBE("stream_read", R_STREAM, W_NONE, 4, 0),
    KDB_PROBE("stream_write", R_NONE, W_STREAM, 0, 4),
    KDB_PROBE("pages_1k_read", R_PAGES, W_NONE, 4, 0),                         // the histogram pass: whole 1 KiB pages, four in flight per wave
    KDB_PROBE("lines_64_write", R_NONE, W_LINES_SC1, 0, 2),                     // what rounds 2-4 wrote
    KDB_PROBE("pieces_128_write", R_NONE, W_CHUNK128_SC1, 0, 2),                // what round 5 writes
    KDB_PROBE("scatter_64", R_STREAM, W_LINES_SC1, 1, 2),                       // one-level scatter: 1 KiB of residues in per 2 KiB of elements out
    KDB_PROBE("scatter_128", R_STREAM, W_CHUNK128_SC1, 1, 2),
    KDB_PROBE("level1_64", R_STREAM, W_LINES_SC1, 1, 3),                        // level 1: 3 bytes out per residue
    KDB_PROBE("level1_128", R_STREAM, W_CHUNK128_SC1, 1, 3),
    KDB_PROBE("level2_64", R_PAGES15, W_LINES_SC1, 2, 2),                       // level 2: two 1.5 KiB pages in per 2 KiB out
    KDB_PROBE("level2_128", R_PAGES15, W_CHUNK128_SC1, 2, 2),
};
#undef KDB_PROBE
constexpr int N_PROBES = (int)(sizeof(PROBES) / sizeof(PROBES[0]));
}  // namespace

extern "C" {

int kdb_hbm_pattern_count(void) { return N_PROBES; }

const char *kdb_hbm_pattern_name(int i) { return (i >= 0 && i < N_PROBES) ? PROBES[i].name : ""; }

int kdb_hbm_pattern_probe(int device_id, double *gb_per_s_out, int n_out)
{
    if (!gb_per_s_out || n_out < N_PROBES) return fail(KDB_ERR_ARG, "kdb_hbm_pattern_probe: room for %d results needed", N_PROBES);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(KDB_ERR_ARG, "device_id=%d but %d device(s) visible", device_id, ndev);
    DeviceGuard g(device_id);
    const uint64_t region = 4ull << 30;                  // far beyond the 256 MB memory-side cache: every piece is written (read) once
    uint8_t *src = nullptr, *dst = nullptr; uint32_t *sink = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    int rc = KDB_OK;
    if (hipMalloc((void **)&src, region) != hipSuccess || hipMalloc((void **)&dst, region) != hipSuccess || hipMalloc((void **)&sink, 64) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(KDB_ERR_NOMEM, "kdb_hbm_pattern_probe: no room for two regions of 4 GiB");
    } else if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess ||
               hipMemsetAsync(src, 1, region, st) != hipSuccess || hipMemsetAsync(dst, 0, region, st) != hipSuccess) {
        rc = fail(KDB_ERR_HIP, "kdb_hbm_pattern_probe: setup failed");
    } else {
        for (int i = 0; i < N_PROBES && rc == KDB_OK; i++) {
            const uint64_t per_step = 512ull * 8ull * ((uint64_t)PROBES[i].read_bytes + PROBES[i].write_bytes);
            const uint32_t steps = (uint32_t)(6.0e9 / (double)per_step) + 1;
            float best = 1e30f;
            for (int rep = 0; rep < 3; rep++) {
                (void)hipEventRecord(a, st);
                PROBES[i].launch(src, region, dst, region, steps, sink, st);
                (void)hipEventRecord(b, st);
                if (hipEventSynchronize(b) != hipSuccess) { rc = fail(KDB_ERR_HIP, "kdb_hbm_pattern_probe: pattern '%s' failed", PROBES[i].name); break; }
                float ms = 0;
                (void)hipEventElapsedTime(&ms, a, b);
                if (rep && ms < best) best = ms;
            }
            gb_per_s_out[i] = (double)steps * (double)per_step / 1e6 / (double)best;
        }
    }
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (st) (void)hipStreamDestroy(st);
    if (src) (void)hipFree(src);
    if (dst) (void)hipFree(dst);
    if (sink) (void)hipFree(sink);
    return rc;
}

}  // extern "C"
