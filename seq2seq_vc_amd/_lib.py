"""ctypes binding of libs2svc_hip.so.  The C ABI is declared in include/s2svc_hip.h and nowhere else: argument lists, return types and
struct layouts are read from that header at import (_abi.py), so a new entry point is declared there, defined in csrc/ and called.

There is deliberately NO fallback: if the shared object is missing or fails to load, importing
any compute op raises.  `build_library()` (used by `__graft_entry__.build()`) cross-compiles the
HIP sources for gfx950 with hipcc; it needs no GPU.
"""
import ctypes
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# S2SVC_LIB: load another build of the SAME library (A/B timing of two kernel variants on one GPU box)
LIB_PATH = os.environ.get("S2SVC_LIB") or os.path.join(CSRC, "libs2svc_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


DEBUG_EXEC_LIB_PATH = os.path.join(CSRC, "libs2svc_hip_dbgexec.so")


def build_library(force=False, verbose=True, debug_exec=False):
    """Compile csrc/*.hip -> csrc/libs2svc_hip.so for gfx950 (in-tree, so it travels to the GPU box).
    debug_exec: the same sources with -DS2SVC_DEBUG_EXEC (common.h: the DPP / v_permlane swap reductions trap when EXEC is not all
    ones) -> csrc/libs2svc_hip_dbgexec.so, loaded through S2SVC_LIB by the GPU case `debug_exec_build_runs_clean` only."""
    lib_path = DEBUG_EXEC_LIB_PATH if debug_exec else LIB_PATH
    if not debug_exec and os.environ.get("S2SVC_LIB"):
        lib_path = os.path.join(CSRC, "libs2svc_hip.so")        # never build over an alternative library named by S2SVC_LIB
    srcs = [os.path.join(CSRC, f) for f in sources()]
    deps = srcs + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [
        os.path.join(_HERE, "..", "include", "s2svc_hip.h")]
    if not force and os.path.exists(lib_path):
        newest = max(os.path.getmtime(p) for p in deps)
        if os.path.getmtime(lib_path) >= newest:
            return lib_path
    objdir = os.path.join(CSRC, "build", "dbgexec") if debug_exec else os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        hdr_time = max(os.path.getmtime(p) for p in deps[len(srcs):])
        if (not force and os.path.exists(obj) and os.path.getmtime(obj) >= os.path.getmtime(src)
                and os.path.getmtime(obj) >= hdr_time):
            return obj
        # -fno-slp-vectorize: no compiler-formed packed-fp32 (v_pk_fma_f32 / v_pk_mul_f32 with op_sel operand swizzles).
        # With them the spline-gradient kernel of the duration predictor returned, a few times per thousand launches and
        # only while another stream kept the chip busy, a wrong element in the last partially active 16-lane row of a wave
        # (same inputs, different output); without them 0 of 800 full AAS-VC steps differ (DESIGN.md section 5 "Hazard"; profiles/AB_LOG.md).
        # The step times are unchanged (the arithmetic that matters is MFMA and explicit 16-byte memory operations).
        # -fno-vectorize: the loop vectoriser forms the same packed operations in a few element-wise kernels.
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-fno-slp-vectorize",
               "-fno-vectorize", "-c", src, "-o", obj]
        if debug_exec:
            cmd.insert(2, "-DS2SVC_DEBUG_EXEC")
        if verbose:
            print("[s2svc build]", " ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        objs = list(ex.map(compile_one, srcs))
    cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", lib_path] + objs
    if verbose:
        print("[s2svc build]", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return lib_path


TORCH_OPS_LIB_PATH = os.path.join(CSRC, "libs2svc_torch_ops.so")


def build_torch_ops(force=False, verbose=True):
    """csrc/torch_ops.cpp -> csrc/libs2svc_torch_ops.so: the TORCH_LIBRARY registration of the kernels (torch.ops.s2svc.*).  Host-only
    C++ against the torch headers, linked to libs2svc_hip.so (found at run time beside it: rpath $ORIGIN); g++, ~20 s."""
    import torch
    from torch.utils import cpp_extension as E
    src = os.path.join(CSRC, "torch_ops.cpp")
    deps = [src, os.path.join(_HERE, "..", "include", "s2svc_hip.h")]
    if not force and os.path.exists(TORCH_OPS_LIB_PATH) and os.path.getmtime(TORCH_OPS_LIB_PATH) >= max(os.path.getmtime(p) for p in deps):
        return TORCH_OPS_LIB_PATH
    tlib = E.library_paths()[0]
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}"]
    cmd += [f"-I{p}" for p in E.include_paths()] + ["-I/opt/rocm/include", src, "-o", TORCH_OPS_LIB_PATH,
                                                    f"-L{tlib}", "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip", "-ltorch_hip",
                                                    f"-L{CSRC}", "-ls2svc_hip", "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{tlib}"]
    if verbose:
        print("[s2svc build]", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return TORCH_OPS_LIB_PATH


c_i32, c_i64, c_f32, c_u64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p


# Signatures and structs come from the header, read once here (_abi.py): an import that succeeds has understood every declaration.
# Every pointer argument is c_void_p (pass ctypes.byref(...), an address or None).  The ABI structs become the classes Operand, GemmDesc,
# ColreduceItem, ScalarTerms, Gather3Job, DerivedJob and Conv1dWgradItem of this module, a C field named like a Python keyword
# getting a trailing underscore (`in_`).
_FUNCTIONS, _STRUCTS = _abi.read_header()
globals().update(_STRUCTS)

_lib = None


def exported_symbols():
    """Every function include/s2svc_hip.h declares, as the parser of _abi.py read them."""
    return sorted(_FUNCTIONS)


def lib():
    """Load the shared object (once).  Raises if it is absent -- there is no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must be imported FIRST: it carries its own libamdhip64; loading ours afterwards makes the
    # dynamic linker bind this library to the SAME HIP runtime instance (one device context, shared streams).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the seq2seq-vc HIP kernels are not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc, no GPU). "
            "There is no CPU fallback for the product path.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _FUNCTIONS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        msg = lib().s2svc_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")
