// classify.hip -- where an operand lives: one HSA pointer query, HIP's own
// query behind it, and the per-thread table of kept host verdicts
// (declared in shim_ctx.hpp; MPIR_Hip_reduce and its kin route on the answer).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <vector>

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include "shim_ctx.hpp"

namespace mpir_hip {

// Whether this process has started the GPU runtime.  HIP runs on the HSA
// runtime, and device or pinned memory exists only once it is open, so until
// then every pointer is pageable host memory and the call needs no HIP query:
// a CPU-only program linked against libmpi with this drop-in never opens
// /dev/kfd for its host-buffer reductions, as MPICH's loop (opsum.c:21-76)
// never does.  hsa_system_get_info answers HSA_STATUS_ERROR_NOT_INITIALIZED
// without starting anything (ROCr's API table is bound when the library loads;
// measured: tools/kfd_probe.py), ~2 ns a call; once open, the answer is cached.
bool gpu_runtime_started() {
    static std::atomic<bool> up{false};
    if (up.load(std::memory_order_relaxed)) return true;
    uint16_t major = 0;
    if (hsa_system_get_info(HSA_SYSTEM_INFO_VERSION_MAJOR, &major) != HSA_STATUS_SUCCESS) return false;
    up.store(true, std::memory_order_relaxed);
    return true;
}

namespace {

// HIP's view of a pointer (100-165 ns a query once HIP is up:
// profiles/r05/classify_cost.log)
Loc classify_hip(const void *p, int *dev) {
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return LOC_HOST;
    }
    if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeUnified) {
        *dev = at.device;
        return LOC_DEVICE;
    }
    if (at.type != hipMemoryTypeHost) return LOC_HOST;
    *dev = at.device;       // the device whose context allocated (registered) it
    return LOC_PINNED;
}

// HIP device ordinal of each HSA GPU agent, matched by PCI domain, bus and
// device (HIP_VISIBLE_DEVICES may hide and renumber agents HSA still lists).
// Empty when any visible device matches no agent or more than one (e.g. a
// partition mode sharing one BDF): the HSA query then answers nothing.
struct AgentMap {
    int n = 0;
    uint64_t handle[kMaxDev];
    int dev[kMaxDev];
    int ncpu = 0;
    uint64_t cpu[kMaxDev];      // CPU agents (owners of host pools)
};
const AgentMap &agent_map() {
    static const AgentMap m = [] {
        AgentMap am;
        struct Gpu { uint64_t handle; uint32_t bdf, domain; };
        std::vector<Gpu> gpus;
        (void)hsa_iterate_agents([](hsa_agent_t a, void *v) {
            hsa_device_type_t t;
            if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
            if (t == HSA_DEVICE_TYPE_CPU) {
                // a CPU agent: bdf 0xffffffff marks it (domain unused)
                static_cast<std::vector<Gpu> *>(v)->push_back(Gpu{a.handle, ~0u, ~0u});
                return HSA_STATUS_SUCCESS;
            }
            if (t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
            Gpu g{a.handle, 0, 0};
            if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &g.bdf) != HSA_STATUS_SUCCESS ||
                hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &g.domain) != HSA_STATUS_SUCCESS)
                return HSA_STATUS_SUCCESS;
            static_cast<std::vector<Gpu> *>(v)->push_back(g);
            return HSA_STATUS_SUCCESS;
        }, &gpus);
        for (const Gpu &g : gpus)
            if (g.bdf == ~0u && g.domain == ~0u && am.ncpu < kMaxDev) am.cpu[am.ncpu++] = g.handle;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || ndev > kMaxDev) {
            (void)hipGetLastError();
            am.n = 0;
            return am;
        }
        for (int d = 0; d < ndev; ++d) {
            int dom = 0, bus = 0, slot = 0;
            if (hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, d) != hipSuccess ||
                hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, d) != hipSuccess ||
                hipDeviceGetAttribute(&slot, hipDeviceAttributePciDeviceId, d) != hipSuccess) {
                (void)hipGetLastError();
                am.n = 0;
                return am;
            }
            int hits = 0;
            for (const Gpu &g : gpus)
                if (g.bdf != ~0u && g.domain == (uint32_t)dom && ((g.bdf >> 8) & 0xff) == (uint32_t)bus &&
                    ((g.bdf >> 3) & 0x1f) == (uint32_t)slot) {
                    am.handle[am.n] = g.handle;
                    am.dev[am.n] = d;
                    ++hits;
                }
            if (hits != 1) {
                am.n = 0;
                return am;
            }
            ++am.n;
        }
        return am;
    }();
    return m;
}

int agent_device(hsa_agent_t a) {
    const AgentMap &m = agent_map();
    for (int i = 0; i < m.n; ++i)
        if (m.handle[i] == a.handle) return m.dev[i];
    return -1;
}

bool cpu_agent(hsa_agent_t a) {
    const AgentMap &m = agent_map();
    for (int i = 0; i < m.ncpu; ++i)
        if (m.cpu[i] == a.handle) return true;
    return false;
}

}  // namespace

// Device memory (hipMalloc, stream-ordered pools, VMM mappings, IPC imports,
// managed) is combined in place; host memory (pageable or pinned) takes the
// host combine, the pinned slot or staging.  One HSA pointer query (24-66 ns
// against HIP's 100-165, profiles/r05/classify_cost.log) answers for memory HSA
// knows as a GPU's: allocations of its pools (HSA), its virtual-memory mappings
// (HSA_VMEM: stream-ordered pools, hipMemCreate + hipMemMap) and IPC imports
// (hsa_ext_amd.h:2344-2372).  Every other answer asks HIP: host pools
// (hipHostMalloc: pinned, whose owning device orders the caller's null-stream
// work before the read), RESERVED_ADDR, graphics interop -- and UNKNOWN, which
// is pageable memory, memory registered with hipHostRegister (HIP registers it
// without HSA's lock), but also managed memory (hipMallocManaged answers
// RESERVED_ADDR in a plain C process, UNKNOWN in a Python process that also
// loaded torch's bundled ROCm runtime: profiles/r05/classify_cost.log,
// classify_diag.log).  For host
// pages -- UNKNOWN, LOCKED, or an allocation owned by a CPU agent -- HIP's host
// verdicts (pageable, pinned) are kept per thread, keyed by the 4 KiB page: the
// next call on the same host buffers costs the HSA query and a lookup.  Only
// host verdicts are kept, and only looked up behind one of those answers, so a
// stale one never sends host memory to a kernel: a page that later becomes a GPU
// allocation answers HSA as the GPU's, and one that becomes managed memory is
// host-accessible (the host path reads it correctly); a device verdict is never
// reused.  What a stale host verdict can change is the host path's choice, since
// HSA reports pages pinned by hipHostRegister as UNKNOWN before and after: a
// page registered after its verdict was kept would be bounced like pageable
// memory instead of DMA'd.  So only calls that cannot reach the staged pipeline
// (`reuse`, verdict_reusable below: within both the mixed slot's and the host
// combine's limits, where pinned and pageable differ only in the null-stream
// ordering) take a kept verdict; a larger call asks HIP again and refreshes it.
// And because the page, not the buffer, keys the table (a registered buffer
// may share its first page with a pageable one classified earlier, or be
// registered after its verdict was kept: ADVICE r5), a call that took a kept
// host verdict (`*kept`) orders its host reads after the null stream whatever
// the verdict says -- the one thing pinned and pageable differ in there.
Loc classify(const void *p, int *dev, bool reuse, bool *kept) {
    if (kept) *kept = false;
    if (!gpu_runtime_started()) return LOC_HOST;
    hsa_amd_pointer_info_t info;
    info.size = sizeof info;
    const bool known = hsa_amd_pointer_info(p, &info, nullptr, nullptr, nullptr) == HSA_STATUS_SUCCESS;
    if (known && (info.type == HSA_EXT_POINTER_TYPE_HSA || info.type == HSA_EXT_POINTER_TYPE_HSA_VMEM ||
                  info.type == HSA_EXT_POINTER_TYPE_IPC)) {
        const int d = agent_device(info.agentOwner);
        if (d >= 0) {
            *dev = d;
            return LOC_DEVICE;
        }
    }
    const bool host_page = known && (info.type == HSA_EXT_POINTER_TYPE_UNKNOWN ||
                                     info.type == HSA_EXT_POINTER_TYPE_LOCKED ||
                                     (info.type == HSA_EXT_POINTER_TYPE_HSA && cpu_agent(info.agentOwner)));
    if (!host_page) return classify_hip(p, dev);
    const uintptr_t page = reinterpret_cast<uintptr_t>(p) >> 12;
    HostVerdict &v = ctx().verdict[(page ^ (page >> 7)) & (kVerdicts - 1)];
    if (reuse && v.page == page) {
        *dev = v.dev;
        if (kept) *kept = true;
        return (Loc)v.loc;
    }
    const Loc l = classify_hip(p, dev);
    if (l != LOC_DEVICE) {
        v.page = page;
        v.loc = l;
        v.dev = l == LOC_PINNED ? *dev : 0;
    } else if (v.page == page) {
        v.page = ~(uintptr_t)0;
    }
    return l;
}

// classify() for the many pointers of one batch.  Its segments usually sit in
// a few allocations (the blocks of one receive buffer, a bucket's tensors in
// one flat buffer), and the query is most of a small batch's host time (two per
// segment, 24-66 ns each): a pointer inside the device allocation that answered
// last -- HSA's own base and size for it -- is that device's without a query.
// Only device answers are kept, for the length of one call (DeviceSpan).
Loc classify_in_span(const void *p, int *dev, DeviceSpan &span) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (a >= span.lo && a < span.hi) {
        *dev = span.dev;
        return LOC_DEVICE;
    }
    const Loc l = classify(p, dev);
    if (l != LOC_DEVICE) return l;
    hsa_amd_pointer_info_t info;
    info.size = sizeof info;
    if (hsa_amd_pointer_info(p, &info, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS) return l;
    if (info.type != HSA_EXT_POINTER_TYPE_HSA && info.type != HSA_EXT_POINTER_TYPE_HSA_VMEM) return l;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(info.agentBaseAddress);
    if (lo && a >= lo && a - lo < info.sizeInBytes && agent_device(info.agentOwner) == *dev) {
        span.lo = lo;
        span.hi = lo + info.sizeInBytes;
        span.dev = *dev;
    }
    return l;
}

bool verdict_reusable(uint64_t bytes) { return bytes <= mixed_max_bytes() && bytes <= host_max_bytes(); }

// devices visible to this process (0 on a CPU-only rank: host operands are
// still combined there, as the reference's loop runs anywhere)
int device_count() {
    static const int n = [] {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess) { (void)hipGetLastError(); c = 0; }
        return c;
    }();
    return n;
}

}  // namespace mpir_hip
