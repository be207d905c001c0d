// host_env_check -- the shim's host-only code (csrc/hip/host_env.hip) checked
// on its own: built with -fsanitize=address,undefined by
// tests/test_host_env_cpu.py, which also makes the /proc and /sys trees under
// argv[1] that the cgroup functions are pointed at:
//   lists/    cpulist files (a, one, empty, big)
//   v1/       /proc/self/cgroup with the v1 lines, no cgroup files
//   hybrid/   the same plus the v2 line
//   deep/     cpuset three levels down (the file two levels up and at the
//             mount), cpu quota at the leaf and a smaller one at its parent
//   noquota/  a cpu controller whose quota is -1, no cpuset controller
// Prints one line per failed check; exit status 1 if any failed.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "host_env.hpp"

using namespace mpir_hip;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

typedef std::vector<int> Ints;
typedef std::vector<std::string> Strs;

static void check_parse_cpulist(const std::string &dir) {
    Ints v;
    CHECK(parse_cpulist((dir + "/a").c_str(), v) == 0 && v == (Ints{0, 1, 2, 3, 8, 10, 11}));
    v.clear();
    CHECK(parse_cpulist((dir + "/one").c_str(), v) == 0 && v == (Ints{5}));
    v.clear();
    // an empty file: fgets reads nothing, which the parser reports like a file it could not open
    CHECK(parse_cpulist((dir + "/empty").c_str(), v) == -1 && v.empty());
    CHECK(parse_cpulist((dir + "/missing").c_str(), v) == -1 && v.empty());
    // a range that runs past CPU_SETSIZE ends at the last CPU a cpu_set_t holds
    CHECK(parse_cpulist((dir + "/big").c_str(), v) == 0);
    Ints want;
    for (int c = CPU_SETSIZE - 4; c < CPU_SETSIZE; ++c) want.push_back(c);
    CHECK(v == want);
}

static void check_cgroup_chain() {
    CHECK(cgroup_chain("/sys/fs/cgroup/cpuset/jobs/a", "/sys/fs/cgroup/cpuset") ==
          (Strs{"/sys/fs/cgroup/cpuset/jobs/a", "/sys/fs/cgroup/cpuset/jobs", "/sys/fs/cgroup/cpuset"}));
    CHECK(cgroup_chain("/somewhere/else", "/sys/fs/cgroup/cpuset") == (Strs{"/sys/fs/cgroup/cpuset"}));
}

static void check_own_cgroup(const std::string &base) {
    for (const char *tree : {"/v1", "/hybrid"}) {       // in a hybrid file the v1 answer wins
        const std::string root = base + tree;
        CHECK(own_cgroup(root, "cpu") == "/sys/fs/cgroup/cpu/jobs/x");
        CHECK(own_cgroup(root, "cpuset") == "/sys/fs/cgroup/cpuset/jobs");
    }
    CHECK(own_cgroup(base + "/v1", "memory") == "");
    CHECK(own_cgroup(base + "/nowhere", "cpu") == "");
}

static void check_cpus_and_quota(const std::string &base) {
    // cpuset.effective_cpus only at an ancestor (and at the mount): the nearest one's count
    CHECK(online_cpus(base + "/deep", 3) == 7);
    // 400000 / 100000 at the leaf, 200000 / 100000 at its parent: the smallest
    CHECK(cgroup_quota_cpus(base + "/deep") == 2);
    CHECK(cgroup_quota_cpus(base + "/noquota") == 0);        // quota -1
    CHECK(cgroup_quota_cpus(base + "/nowhere") == 0);
    // no cpuset controller, or one without a file anywhere: the mask
    CHECK(online_cpus(base + "/noquota", 12) == 12);
    CHECK(online_cpus(base + "/v1", 9) == 9);
    CHECK(online_cpus(base + "/v1", 0) == 1);
}

static void check_share_threads() {
    CHECK(share_threads(16, 16, 0, 1) == 16);
    CHECK(share_threads(64, 64, 0, 8) == 8);
    CHECK(share_threads(16, 256, 16, 8) == 2);
    CHECK(share_threads(128, 256, 0, 2) == 16);
    CHECK(share_threads(4, 4, 0, 16) == 1);
    CHECK(share_threads(256, 256, 0, 1) == 16);
    CHECK(share_threads(8, 8, 3, 1) == 3);
}

static void check_cvar_long() {
    const char *chunk = "MPIR_CVAR_REDUCE_LOCAL_STAGE_CHUNK_MB", *keep = "MPIR_CVAR_REDUCE_LOCAL_KEEP_MIN_MB";
    unsetenv(chunk);
    unsetenv(keep);
    CHECK(cvar_long(chunk, 1, 1024, 16) == 16);
    CHECK(cvar_long(keep, 0, 4096, 16) == 16);
    struct { const char *text; long chunk, keep; } cases[] = {
        {"32", 32, 32}, {"1", 1, 1}, {"1024", 1024, 1024}, {"4096", 16, 4096},     // in range, the ends
        {"0", 16, 0}, {"-1", 16, 16},                                               // below
        {"1025", 16, 1025}, {"4097", 16, 16},                                       // above
        {"abc", 16, 0},                                                             // no number reads as 0
    };
    for (const auto &c : cases) {
        setenv(chunk, c.text, 1);
        setenv(keep, c.text, 1);
        CHECK(cvar_long(chunk, 1, 1024, 16) == c.chunk);
        CHECK(cvar_long(keep, 0, 4096, 16) == c.keep);
    }
    unsetenv(chunk);
    unsetenv(keep);
}

static void check_copy_pool() {
    // (never destroyed, as in the library: its idle workers wait on it until the process ends)
    static CopyPool *const made = new CopyPool(4, 4);
    CopyPool &pool = *made;
    CHECK(pool.threads() == 4);
    {
        const size_t n = ((size_t)3 << 20) + 17;
        std::vector<char> src(n), dst(n + 1, (char)0x5a);
        uint32_t x = 12345;
        for (char &c : src) c = (char)((x = x * 1664525u + 1013904223u) >> 24);
        pool.copy(dst.data(), src.data(), n, (size_t)1 << 20);
        CHECK(memcmp(dst.data(), src.data(), n) == 0);
        CHECK(dst[n] == (char)0x5a);
    }
    {
        std::atomic<int> calls[37] = {};
        pool.run(37, [](void *p, size_t k) { ++static_cast<std::atomic<int> *>(p)[k]; }, calls);
        for (const auto &c : calls) CHECK(c.load() == 1);
    }
    {
        // Thread A holds the job (its part 0 waits for B); B calls run() meanwhile:
        // it finds the workers busy and runs every part itself.
        struct Both {
            std::atomic<bool> a_started{false}, b_done{false};
            std::atomic<int> a_calls[8] = {}, b_calls[8] = {};
            std::atomic<int> b_elsewhere{0};
            std::thread::id b_id;
        } s;
        std::thread a([&] {
            pool.run(8, [](void *p, size_t k) {
                Both *s = static_cast<Both *>(p);
                ++s->a_calls[k];
                if (k == 0) {
                    s->a_started = true;
                    while (!s->b_done) std::this_thread::yield();
                }
            }, &s);
        });
        std::thread b([&] {
            s.b_id = std::this_thread::get_id();
            while (!s.a_started) std::this_thread::yield();
            pool.run(8, [](void *p, size_t k) {
                Both *s = static_cast<Both *>(p);
                ++s->b_calls[k];
                if (std::this_thread::get_id() != s->b_id) ++s->b_elsewhere;
            }, &s);
            s.b_done = true;
        });
        a.join();
        b.join();
        for (int k = 0; k < 8; ++k) CHECK(s.a_calls[k] == 1 && s.b_calls[k] == 1);
        CHECK(s.b_elsewhere == 0);
    }
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <directory of fake trees>\n", argv[0]);
        return 2;
    }
    const std::string base = argv[1];
    check_parse_cpulist(base + "/lists");
    check_cgroup_chain();
    check_own_cgroup(base);
    check_cpus_and_quota(base);
    check_share_threads();
    check_cvar_long();
    check_copy_pool();
    printf("%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
