"""Build libsphx.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

Every .hip source is compiled to its own object (in parallel, rebuilt only when it or a header is
newer) and the objects are linked into sph-code_amd/libsphx.so."""
import fcntl
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, ".obj")
LIB = os.path.join(HERE, "libsphx.so")
SOURCES = ["sphx_api.hip", "sphx_grid.hip", "sphx_knn.hip", "sphx_knn_group.hip", "sphx_sums.hip",
           "sphx_integrate.hip", "sphx_loopforms.hip", "sphx_dev.hip", "sphx_refresh.hip", "sphx_blob.hip",
           "sphx_agb.hip", "sphx_gravity.hip", "sphx_arb.hip", "sphx_rad.hip", "sphx_cool.hip",
           "sphx_dust.hip", "sphx_chem.hip", "sphx_phase.hip", "sphx_radphase.hip", "sphx_side.hip", "sphx_sn.hip",
           "sphx_insert.hip", "sphx_scale.hip", "sphx_census.hip", "sphx_map.hip"]
HEADERS = [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
          [os.path.join(os.path.dirname(HERE), "include", "sphx.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# per source: the grouped search kernel schedules better with loads clustered (LLVM's max-memory-clause strategy:
# knn_group_kernel 0.443 -> 0.433 ms at 1e6 particles; the sum passes and the general kernel lose 1-3 % with it)
FILE_FLAGS = {"sphx_knn_group.hip": ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]}


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libsphx.so cannot be built (set HIPCC=/path/to/hipcc)")


def _sources():
    return [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def _flag_stamp(extra):
    return " ".join(FLAGS + extra) + " | " + repr(sorted(FILE_FLAGS.items()))


def _extra_flags():
    """SPHX_EXTRA_FLAGS: further hipcc flags for every source, e.g. -DKNN_MIN_WAVES=5 to try another value of a
    compile-time tuning constant."""
    return os.environ.get("SPHX_EXTRA_FLAGS", "").split()


def needs_build():
    if not os.path.exists(LIB):
        return True
    stamp_file = os.path.join(OBJ, "flags.txt")
    if os.path.exists(stamp_file) and open(stamp_file).read() != _flag_stamp(_extra_flags()):
        return True                      # same sources, other flags
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in _sources()] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(hipcc, src, obj, extra, verbose):
    tmp = "%s.%d.tmp" % (obj, os.getpid())
    cmd = [hipcc] + FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + extra + ["-c", "-o", tmp, src]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s%s" % (src, res.stdout, res.stderr))
    os.replace(tmp, obj)
    return res.stderr


def build(force=False, verbose=False):
    """Compile every HIP source into sph-code_amd/libsphx.so.  Returns the library path."""
    if not force and not needs_build():
        return LIB
    hipcc = hipcc_path()
    os.makedirs(OBJ, exist_ok=True)
    # one builder at a time (ranks under torch.distributed.run, pytest-xdist workers, a variants script beside a test run);
    # whoever waited finds the work done
    with open(os.path.join(OBJ, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not needs_build():
            return LIB
        return _build_locked(hipcc, force, verbose)


def _build_locked(hipcc, force, verbose):
    extra = _extra_flags()
    stamp_file = os.path.join(OBJ, "flags.txt")
    same_flags = os.path.exists(stamp_file) and open(stamp_file).read() == _flag_stamp(extra)
    hdr_t = max(os.path.getmtime(h) for h in HEADERS)
    jobs, objs = [], []
    for s in _sources():
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s.replace(".hip", ".o"))
        objs.append(obj)
        stale = force or not same_flags or not os.path.exists(obj) or \
            os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_t)
        if stale:
            jobs.append((src, obj))
    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        for warn in ex.map(lambda j: _compile(hipcc, j[0], j[1], extra, verbose), jobs):
            if verbose and warn.strip():
                print(warn)
    open(stamp_file, "w").write(_flag_stamp(extra))
    tmp = "%s.%d.tmp" % (LIB, os.getpid())
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("link failed:\n" + res.stdout + res.stderr)
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    import sys
    print(build(force="--force" in sys.argv, verbose=True))
