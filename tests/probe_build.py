"""The one builder of the CPU tests' probes: a few sources (a tests/*_probe.cpp, sometimes uhc_plan.cpp beside it) -> uhc_amd/csrc/build/<name> with the HOST
compiler ($CXX, else g++): no hipcc, no HIP runtime.  Rebuilt when a source or a listed dependency is newer; written under a per-process name and renamed into
place, so that two test processes never load a half-written file."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uhc_amd", "csrc")
# for the probes that read the struct definitions of uhc_device.h / uhc_host.h: the HIP headers, nothing of the runtime
HIP_STRUCT_FLAGS = ("-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
# products and sums rounded separately, as the device units are compiled
NO_CONTRACT = ("-ffp-contract=off",)


def build_probe(name, sources, deps=(), flags=()):
    """name: the file under uhc_amd/csrc/build -- a shared library when it ends in .so, a program otherwise; sources, deps: paths below the repository root
    (deps: the headers whose edit rebuilds the probe); flags: what this probe adds to -std=c++17 -O1 -I<csrc>.  Returns the path of what was built."""
    out_dir = os.path.join(CSRC, "build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, name)
    srcs = [os.path.join(ROOT, s) for s in sources]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in srcs + [os.path.join(ROOT, d) for d in deps]):
        tmp = out + f".{os.getpid()}.tmp"
        shared = ["-fPIC", "-shared", "-fvisibility=hidden"] if name.endswith(".so") else []
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", *shared, "-I" + CSRC, *flags, *srcs, "-o", tmp])
        os.replace(tmp, out)
    return out
