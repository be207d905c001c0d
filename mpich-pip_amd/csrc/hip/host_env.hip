// host_env.hip -- the host-only part of the shim (host_env.hpp): environment
// knobs, the size of the copy / host-combine pool from launcher variables,
// affinity, cgroup cpuset and quota, and NUMA placement.  Nothing here includes
// or calls HIP or HSA, so the unit also compiles as plain C++
// (g++ -std=c++17 -x c++ -pthread; tests/progs/host_env_check.cpp links it).
#include <stdio.h>
#include <stdlib.h>
#include <sys/syscall.h>

#include "host_env.hpp"

namespace mpir_hip {

long cvar_long(const char *name, long lo, long hi, long dflt) {
    const char *e = getenv(name);
    if (!e) return dflt;
    const long v = atol(e);
    return v >= lo && v <= hi ? v : dflt;
}

// Ranks of this job on this node (>= 1).  Every rank of a host-buffer
// MPI_Allreduce reaches its combine at the same moment, so the node's CPUs are
// shared by all of them.  Sources, in order: MPIR_Hip_set_local_ranks() (inside
// libmpi the glue passes MPICH's node communicator size, mpich_glue.c), then
// the launcher's environment -- MPI_LOCALNRANKS (Hydra, pmip_cb.c:658-662),
// MPIR_PIP_SIZE (this repo's mpiexec: one node), LOCAL_WORLD_SIZE (torchrun),
// OMPI_COMM_WORLD_LOCAL_SIZE (Open MPI's launcher); none: 1.
std::atomic<int> g_local_ranks{0};
int local_ranks() {
    const int set = g_local_ranks.load(std::memory_order_relaxed);
    if (set > 0) return set;
    static const int env = [] {
        for (const char *k : {"MPI_LOCALNRANKS", "MPIR_PIP_SIZE", "LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE"})
            if (const char *e = getenv(k)) {
                const int n = atoi(e);
                if (n >= 1 && n <= (1 << 20)) return n;
            }
        return 1;
    }();
    return env;
}

// Host-combine threads for one rank, from the CPUs the node's L local ranks
// share (the reference's combine is one thread per rank,
// opsum.c:21-76):
//   * affinity: a mask of m of the c CPUs the job may use (the cgroup's cpuset,
//     else the online CPUs).  Ranks bound to disjoint sets (L * m <= c) each
//     own their mask; unbound ranks (m = c) share it L ways; in between (e.g.
//     --bind-to socket) ceil(L * m / c) ranks share each mask;
//   * cgroup quota q (cpu.max): the job's or container's, shared by all L.
// The share is at most 16 (the host combine's measured scaling: 256 MiB fp32
// SUM, 16-CPU quota, 131-136 GiB/s on 4 threads, 259-299 on 16;
// profiles/archive/r02/host_threads_ab.log).  No floor: with at most one CPU
// per rank the caller combines alone and the library starts no thread, as
// MPICH's loop starts none (8 unbound ranks on this job's 16-CPU quota: one
// worker each beside the caller).  Copies (bounce path, mixed-residency slots)
// keep to at most 4 parts, which already outrun a PCIe upload.
// MPIR_CVAR_REDUCE_LOCAL_STAGE_THREADS sets both (1 = the caller alone).
// (pool_threads() sizes a pool without creating one: the floating pool's
// threads start only when a copy or a combine off the operands' node needs
// them, never beside a NUMA node's pool that does the work; the size is fixed
// at the first call, so MPIR_Hip_set_local_ranks() acts before the first host
// combine)
//
// This process's own cgroup, as /proc/self/cgroup names it: the v2 path ("0::")
// or the v1 path of `controller`; "" if the file or the entry is missing.  The
// cgroup files are read there and up its ancestors (without a
// cgroup namespace -- Slurm on bare metal -- the mount's root files describe
// the whole node, not this job).
std::string own_cgroup(const std::string &root, const char *controller) {
    FILE *f = fopen((root + "/proc/self/cgroup").c_str(), "r");
    if (!f) return "";
    char line[1024];
    std::string v2, v1;
    while (fgets(line, sizeof line, f)) {
        line[strcspn(line, "\n")] = 0;
        char *c1 = strchr(line, ':');
        char *c2 = c1 ? strchr(c1 + 1, ':') : nullptr;
        if (!c2) continue;
        *c2 = 0;
        const char *ctrls = c1 + 1, *path = c2 + 1;
        // (first item: `line` still reads "0:", so this never matches a v2 entry)
        if (!strncmp(line, "0", 2) && !*ctrls) v2 = path;
        for (const char *t = ctrls; *t;) {                  // "cpu,cpuacct"
            const size_t n = strcspn(t, ",");
            if (n == strlen(controller) && !strncmp(t, controller, n)) v1 = path;
            t += n + (t[n] == ',');
        }
    }
    fclose(f);
    return !v1.empty() ? "/sys/fs/cgroup/" + std::string(controller) + v1 : (!v2.empty() ? "/sys/fs/cgroup" + v2 : "");
}
// dir and its ancestors up to the mount point (inclusive), innermost first
std::vector<std::string> cgroup_chain(const std::string &dir, const char *mount) {
    std::vector<std::string> out;
    std::string d = dir;
    while (d.size() > strlen(mount) && d.compare(0, strlen(mount), mount) == 0) {
        while (d.size() > 1 && d.back() == '/') d.pop_back();
        out.push_back(d);
        d = d.substr(0, d.rfind('/'));
    }
    out.push_back(mount);
    return out;
}
// The CPUs the job's ranks can share: this process's cgroup cpuset (a
// container pinned to 16 of the host's 256 CPUs gives every unbound rank that
// same 16-CPU mask), read at its own cgroup or the nearest ancestor that has
// one.  If no cpuset can be found, `mask` (this process's affinity): the L
// local ranks are then taken to share it, the conservative reading.
int online_cpus(const std::string &root, int mask) {
    const std::string v1 = own_cgroup(root, "cpuset");
    const bool is_v1 = v1.compare(0, 22, "/sys/fs/cgroup/cpuset/") == 0 || v1 == "/sys/fs/cgroup/cpuset";
    const char *mount = is_v1 ? "/sys/fs/cgroup/cpuset" : "/sys/fs/cgroup";
    const char *file = is_v1 ? "/cpuset.effective_cpus" : "/cpuset.cpus.effective";
    if (!v1.empty())
        for (const std::string &d : cgroup_chain(v1, mount)) {
            std::vector<int> cpus;
            if (parse_cpulist((root + d + file).c_str(), cpus) == 0 && !cpus.empty()) return (int)cpus.size();
        }
    return mask >= 1 ? mask : 1;
}
// the cgroup's CPU quota in CPUs (v2 cpu.max "quota period", v1 cfs_quota_us /
// cfs_period_us) -- the smallest along this process's cgroup and its
// ancestors -- 0 if none
int cgroup_quota_cpus(const std::string &root) {
    const std::string own = own_cgroup(root, "cpu");
    if (own.empty()) return 0;
    const bool is_v1 = own.compare(0, 19, "/sys/fs/cgroup/cpu/") == 0 || own == "/sys/fs/cgroup/cpu";
    long best = 0;
    for (const std::string &d : cgroup_chain(own, is_v1 ? "/sys/fs/cgroup/cpu" : "/sys/fs/cgroup")) {
        long quota = -1, period = 0;
        if (!is_v1) {
            if (FILE *f = fopen((root + d + "/cpu.max").c_str(), "r")) {
                char q[32];
                if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
                fclose(f);
            }
        } else if (FILE *fq = fopen((root + d + "/cpu.cfs_quota_us").c_str(), "r")) {
            if (fscanf(fq, "%ld", &quota) != 1) quota = -1;
            fclose(fq);
            if (FILE *fp = fopen((root + d + "/cpu.cfs_period_us").c_str(), "r")) {
                if (fscanf(fp, "%ld", &period) != 1) period = 0;
                fclose(fp);
            }
        }
        if (quota <= 0 || period <= 0) continue;
        const long v = (quota + period - 1) / period;
        if (v >= 1 && v < (1L << 20) && (best == 0 || v < best)) best = v;
    }
    return (int)best;
}
int share_threads(int mask, int online, int quota, int L) {
    if (L < 1) L = 1;
    if (mask < 1) mask = 1;
    if (online < mask) online = mask;
    int sharers = (int)(((long)L * mask + online - 1) / online);
    sharers = std::max(1, std::min(L, sharers));
    int n = mask / sharers;
    if (quota > 0) n = std::min(n, quota / L);
    return std::max(1, std::min(16, n));
}
const char *stage_threads_env() {
    static const char *e = getenv("MPIR_CVAR_REDUCE_LOCAL_STAGE_THREADS");
    return e;
}
int pool_threads() {
    static const int n = [] {
        const char *e = stage_threads_env();
        if (e) {
            const int v = atoi(e);
            return v < 1 || v > 64 ? 4 : v;
        }
        cpu_set_t set;
        const int mask = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : 1;
        return share_threads(mask, online_cpus("", mask), cgroup_quota_cpus(""), local_ranks());
    }();
    return n;
}
CopyPool &copy_pool() {
    static CopyPool *pool = new CopyPool(pool_threads(), stage_threads_env() ? pool_threads() : 4);
    return *pool;
}

// ---- NUMA placement of the host combine ---------------------------------
// A both-host combine is bound by the host's memory bandwidth, and a thread
// reading the other socket's memory runs at about half the rate: torch /
// hipHostMalloc place pinned buffers on the GPU's node while a rank's pageable
// buffers sit wherever it first touched them, and the floating pool then
// reads most of one kind remotely (tools/pinned_read_probe.py,
// profiles/archive/r03/pinned_read_probe.log: the same 256 MiB fp32 SUM at 70-76 GiB/s
// for pinned operands on node 0 against 100-136 for pageable ones on node 1).
// When both operands' sampled pages sit on one node, the split runs on a pool
// confined to that node's CPUs (within the process's affinity mask);
// MPIR_CVAR_REDUCE_LOCAL_HOST_NUMA=0 keeps the floating pool.
bool host_numa_enabled() {
    static const bool on = [] {
        const char *e = getenv("MPIR_CVAR_REDUCE_LOCAL_HOST_NUMA");
        return !(e && atoi(e) == 0);
    }();
    return on;
}

int parse_cpulist(const char *path, std::vector<int> &out) {
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    char buf[4096];
    const bool ok = fgets(buf, sizeof buf, f) != nullptr;
    fclose(f);
    if (!ok) return -1;
    for (char *p = buf; *p && *p != '\n';) {
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        p = end;
        if (*p == '-') {
            b = strtol(p + 1, &end, 10);
            p = end;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) out.push_back((int)c);
        if (*p == ',') ++p;
    }
    return 0;
}

// per NUMA node: the CPUs of this process's affinity mask on it, the first
// hardware thread of every core before the second ones
std::vector<std::vector<int>> read_node_cpus(const std::string &root) {
    std::vector<std::vector<int>> v;
    cpu_set_t mask;
    if (sched_getaffinity(0, sizeof mask, &mask) != 0) return v;
    for (int node = 0; node < 64; ++node) {
        char path[96];
        snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
        std::vector<int> all;
        v.emplace_back();
        if (parse_cpulist((root + path).c_str(), all) != 0) continue;     // node ids need not be contiguous
        std::vector<int> first, second;
        for (int c : all) {
            if (!CPU_ISSET(c, &mask)) continue;
            snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", c);
            std::vector<int> sib;
            (parse_cpulist((root + path).c_str(), sib) == 0 && !sib.empty() && sib[0] != c ? second : first).push_back(c);
        }
        first.insert(first.end(), second.begin(), second.end());
        v.back() = first;
    }
    return v;
}
const std::vector<std::vector<int>> &node_cpus() {
    static const std::vector<std::vector<int>> nodes = read_node_cpus("");
    return nodes;
}

// NUMA nodes with CPUs this process may use
int usable_nodes() {
    static const int n = [] {
        int c = 0;
        for (const auto &cpus : node_cpus()) c += !cpus.empty();
        return c;
    }();
    return n;
}

// the NUMA node holding the sampled pages of both operands (start, middle and
// end of each), or -1 (mixed, not yet touched, or unknown)
int host_node(const void *a, const void *b, size_t bytes) {
    if (bytes == 0 || usable_nodes() < 2) return -1;
    void *pages[6];
    int status[6];
    const uintptr_t base[2] = {reinterpret_cast<uintptr_t>(a), reinterpret_cast<uintptr_t>(b)};
    for (int i = 0; i < 2; ++i) {
        pages[3 * i] = reinterpret_cast<void *>(base[i] & ~(uintptr_t)4095);
        pages[3 * i + 1] = reinterpret_cast<void *>((base[i] + bytes / 2) & ~(uintptr_t)4095);
        pages[3 * i + 2] = reinterpret_cast<void *>((base[i] + bytes - 1) & ~(uintptr_t)4095);
    }
    if (syscall(SYS_move_pages, 0, 6, pages, nullptr, status, 0) != 0) return -1;
    for (int i = 1; i < 6; ++i)
        if (status[i] != status[0]) return -1;
    return status[0] >= 0 && status[0] < (int)node_cpus().size() ? status[0] : -1;
}

// the pool for a both-host combine of `bytes` per operand: pinned to the
// operands' node when they share one (and it has CPUs of ours), else the
// floating pool
CopyPool &combine_pool(const void *a, const void *b, size_t bytes) {
    static std::mutex mu;
    static CopyPool *per_node[64] = {};
    const int node = host_numa_enabled() ? host_node(a, b, bytes) : -1;
    if (node < 0 || node >= 64 || node_cpus()[(size_t)node].size() < 2) return copy_pool();
    std::lock_guard<std::mutex> lk(mu);
    if (!per_node[node]) {
        const std::vector<int> &cpus = node_cpus()[(size_t)node];
        const int n = std::min<int>(pool_threads(), (int)cpus.size());
        // n - 1 workers confined to the node's CPUs and the caller: no more
        // threads than the floating pool (the CPUs the process may use)
        per_node[node] = new CopyPool(n, 4, cpus);
    }
    return *per_node[node];
}

}  // namespace mpir_hip
