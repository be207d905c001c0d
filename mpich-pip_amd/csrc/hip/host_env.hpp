// host_env.hpp -- what the shim learns from, and runs on, the host alone: the
// integer knobs of the environment (cvar_long), the copy / host-combine thread
// pool (CopyPool), its size from the CPUs this rank may use (launcher
// variables, affinity mask, cgroup cpuset and quota) and the NUMA node of a
// both-host combine.  No HIP, no HSA: host_env.hip compiles with a plain C++
// compiler too, and the functions that read /proc and /sys take the root of
// that tree ("" in the library), so a test can hand them one it made
// (tests/test_host_env_cpu.py).
#pragma once
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace mpir_hip {

// The integer environment variable `name`: its atol() value when set and
// within [lo, hi] (text that is no number reads as 0), else dflt.
long cvar_long(const char *name, long lo, long hi, long dflt);

// Host copies of the bounce path, split over a small process-wide pool of
// worker threads: one thread moves 31-33 GB/s between pageable and pinned
// memory on the MI355X host, four 83-86 GB/s (tools/memcpy_bw.cpp,
// profiles/archive/r01s3_memcpy_bw.log) -- more than the ~51 GB/s a PCIe Gen5 x16
// upload takes; the host combine uses every thread (copy_pool() below).
// MPIR_CVAR_REDUCE_LOCAL_STAGE_THREADS (1 = the calling thread alone).  The pool is never torn down: its idle workers end
// with the process, so exit never waits on them.
class CopyPool {
  public:
    // `cpus`: the workers may run on these CPUs only (a NUMA node's pool: the
    // scheduler still balances them over the node); empty: the process's mask
    CopyPool(int nthreads, int copy_parts, std::vector<int> cpus = {})
        : n_(nthreads), copy_n_(std::min(nthreads, copy_parts)), pid_(getpid()) {
        cpu_set_t set;
        CPU_ZERO(&set);
        for (int c : cpus) CPU_SET(c, &set);
        for (int i = 1; i < n_; ++i)
            std::thread([this, set, pin = !cpus.empty()] {
                if (pin) (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
                work();
            }).detach();
    }
    int threads() const { return n_; }
    // fn(ctx, k) for every k < nparts, the parts handed out one at a time to
    // the calling thread and the workers alike, so a slower thread (remote
    // memory, a throttled or preempted CPU) simply takes fewer; returns when
    // all are done.  One job at a time: a caller that finds the workers busy
    // with another thread's job runs its parts alone rather than waiting, so
    // concurrent callers (other devices, other host combines) never serialise
    // behind each other.
    void run(size_t nparts, void (*fn)(void *, size_t), void *ctx) {
        std::unique_lock<std::mutex> job(job_mu_, std::defer_lock);
        // a forked child has none of the workers: run alone there
        if (n_ <= 1 || nparts <= 1 || getpid() != pid_ || !job.try_lock()) {
            for (size_t k = 0; k < nparts; ++k) fn(ctx, k);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = fn;
            ctx_ = ctx;
            nparts_ = nparts;
            next_ = 1;                                  // part 0 is the caller's
            pending_ = nparts - 1;
            ++gen_;
        }
        // wake only as many workers as there are parts for (a copy of 4
        // parts on a 16-thread pool: +9 us at 1 MiB with notify_all)
        for (size_t k = 1; k < nparts && k < (size_t)n_; ++k) cv_.notify_one();
        fn(ctx, 0);
        std::unique_lock<std::mutex> lk(mu_);
        while (next_ < nparts_) {
            const size_t k = next_++;
            lk.unlock();
            fn(ctx, k);
            lk.lock();
            --pending_;
        }
        done_.wait(lk, [this] { return pending_ == 0; });
    }
    // copies split into at most copy_n_ parts: PCIe, not the host's memory,
    // bounds them, and more parts only add wake-ups (host->device 1 MiB 52 ->
    // 74 us with 16 parts, profiles/archive/r02/host_threads_ab.log)
    void copy(char *dst, const char *src, size_t bytes, size_t min_split = (size_t)1 << 20) {
        if (copy_n_ <= 1 || bytes < min_split || getpid() != pid_) {
            memcpy(dst, src, bytes);
            return;
        }
        struct C {
            char *d;
            const char *s;
            size_t bytes, part;
        } c{dst, src, bytes, ((bytes + copy_n_ - 1) / copy_n_ + 63) & ~(size_t)63};
        run((bytes + c.part - 1) / c.part, [](void *p, size_t k) {
            const C *c = static_cast<const C *>(p);
            const size_t o = k * c->part;
            memcpy(c->d + o, c->s + o, std::min(c->part, c->bytes - o));
        }, &c);
    }

  private:
    void work() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return gen_ != seen; });
            seen = gen_;
            while (next_ < nparts_) {
                const size_t k = next_++;
                lk.unlock();
                fn_(ctx_, k);
                lk.lock();
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    int n_, copy_n_;
    pid_t pid_;
    std::mutex job_mu_, mu_;
    std::condition_variable cv_, done_;
    void (*fn_)(void *, size_t) = nullptr;
    void *ctx_ = nullptr;
    size_t nparts_ = 0, next_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
};

// ranks of this job on this node (MPIR_Hip_set_local_ranks() stores into
// g_local_ranks; 0: take the launcher's environment)
extern std::atomic<int> g_local_ranks;
int local_ranks();

// the cgroup files under `root` ("" = this machine's own /proc and /sys)
std::string own_cgroup(const std::string &root, const char *controller);
std::vector<std::string> cgroup_chain(const std::string &dir, const char *mount);
int online_cpus(const std::string &root, int mask);
int cgroup_quota_cpus(const std::string &root);

// host-combine threads of one rank, and the pools that run them
int share_threads(int mask, int online, int quota, int L);
const char *stage_threads_env();
int pool_threads();
CopyPool &copy_pool();

// NUMA placement of the host combine
bool host_numa_enabled();
int parse_cpulist(const char *path, std::vector<int> &out);
std::vector<std::vector<int>> read_node_cpus(const std::string &root);
const std::vector<std::vector<int>> &node_cpus();
int usable_nodes();
int host_node(const void *a, const void *b, size_t bytes);
CopyPool &combine_pool(const void *a, const void *b, size_t bytes);

}  // namespace mpir_hip
