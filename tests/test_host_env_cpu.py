"""The shim's host-only code (csrc/hip/host_env.hip: cvar_long, CopyPool, the
cgroup and cpulist parsers, share_threads) on its own: compiled as plain C++
with AddressSanitizer and UBSan together with tests/progs/host_env_check.cpp,
which makes the checks, and run on /proc and /sys trees made here (the parsers
take the root of the tree they read; the library passes "").  No GPU library is
loaded: the program has its own main.

A pure cgroup-v2 /proc/self/cgroup is not among the trees: own_cgroup's v2
branch is moved as it stands (first item) and gets its case with
its fix.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "mpich-pip_amd", "csrc", "hip")

V1 = "4:cpu,cpuacct:/jobs/x\n7:cpuset:/jobs\n"


def put(root, path, text):
    p = os.path.join(str(root), path.lstrip("/"))
    os.makedirs(os.path.dirname(p), exist_ok=True)
    with open(p, "w") as f:
        f.write(text)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_env") / "host_env_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-pthread", "-Wall", "-I" + HIP, "-x", "c++", os.path.join(HIP, "host_env.hip"),
                    os.path.join(ROOT, "tests", "progs", "host_env_check.cpp"), "-o", exe], check=True)
    return exe


def test_host_env(check, tmp_path):
    put(tmp_path, "lists/a", "0-3,8,10-11\n")
    put(tmp_path, "lists/one", "5\n")
    put(tmp_path, "lists/empty", "")
    put(tmp_path, "lists/big", "1020-1030\n")             # CPU_SETSIZE is 1024
    put(tmp_path, "v1/proc/self/cgroup", V1)
    put(tmp_path, "hybrid/proc/self/cgroup", V1 + "0::/init.scope\n")
    cg = "deep/sys/fs/cgroup"
    put(tmp_path, "deep/proc/self/cgroup", "3:cpu,cpuacct:/jobs/x\n9:cpuset:/jobs/a/b\n")
    os.makedirs(os.path.join(str(tmp_path), cg, "cpuset/jobs/a/b"))
    put(tmp_path, cg + "/cpuset/jobs/cpuset.effective_cpus", "0-5,8\n")
    put(tmp_path, cg + "/cpuset/cpuset.effective_cpus", "0-63\n")
    put(tmp_path, cg + "/cpu/jobs/x/cpu.cfs_quota_us", "400000\n")
    put(tmp_path, cg + "/cpu/jobs/x/cpu.cfs_period_us", "100000\n")
    put(tmp_path, cg + "/cpu/jobs/cpu.cfs_quota_us", "200000\n")
    put(tmp_path, cg + "/cpu/jobs/cpu.cfs_period_us", "100000\n")
    put(tmp_path, cg + "/cpu/cpu.cfs_quota_us", "-1\n")
    put(tmp_path, cg + "/cpu/cpu.cfs_period_us", "100000\n")
    put(tmp_path, "noquota/proc/self/cgroup", "3:cpu,cpuacct:/jobs/x\n")
    put(tmp_path, "noquota/sys/fs/cgroup/cpu/jobs/x/cpu.cfs_quota_us", "-1\n")
    put(tmp_path, "noquota/sys/fs/cgroup/cpu/jobs/x/cpu.cfs_period_us", "100000\n")
    r = subprocess.run([check, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "0 checks failed", r.stdout
