"""ctypes binding of the C-ABI library (include/umr.h).  Fails loudly when the
HIP library is missing: there is no CPU / PyTorch fallback in the product path.
Every function's argument and return types are read from the header's prototypes when
this module is imported; only the descriptor structs are mirrored by hand (MIRRORS)."""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(_HERE, "..", "include", "umr.h")   # the file csrc/umr_common.h includes: argument and return types are read from it
LIB_PATH = os.environ.get("UMR_LIB") or os.path.join(_HERE, "lib", "libumr.so")   # UMR_LIB: another build of the library (the fenced split-K one: libumr_fence.so)
CSRC = os.path.join(_HERE, "csrc")

F32, BF16, BF16X3 = 0, 1, 2
EPI_BIAS, EPI_ADD_AUX, EPI_MASK_RELU, EPI_MASK_DGELU, EPI_ADD_AUX2, EPI_OUT_F32, EPI_ROWBIAS, EPI_OUT_X3 = 1, 2, 4, 8, 16, 32, 64, 128
EPI_AUX_X3, EPI_AUX2_X3, EPI_C2_X3 = 256, 512, 1024
ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH = 0, 1, 2, 3
ACT_SIGMOID = 5
F32_EXACT, F32_X3, F32_X3_FAST = 0, 1, 2   # umr_f32_mode

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


class GemmDesc(ctypes.Structure):
    _fields_ = [("A", _vp), ("B", _vp), ("C", _vp), ("C2", _vp), ("bias", _vp), ("aux", _vp),
                ("aux2", _vp), ("rowbias", _vp),
                ("lda", _i64), ("ldb", _i64), ("ldc", _i64), ("ldc2", _i64), ("ldaux", _i64), ("ldaux2", _i64),
                ("M", _i32), ("N", _i32), ("K", _i32), ("dtype", _i32),
                ("flags", _i32), ("act", _i32), ("c2_mode", _i32), ("rows_per_batch", _i32),
                ("conv", _i32), ("nb", _i32), ("H", _i32), ("W", _i32), ("Cin", _i32), ("Ho", _i32), ("Wo", _i32),
                ("a_rows_in", _i32), ("a_rows_out", _i32), ("a_row_off", _i32),
                ("c_rows_in", _i32), ("c_rows_out", _i32), ("c_row_off", _i32), ("aux_mod", _i32),
                ("red_w", _vp), ("red_out", _vp), ("red_c", _i32), ("no_store", _i32)]


class GemmTnDesc(ctypes.Structure):
    _fields_ = [("dY", _vp), ("X", _vp), ("dW", _vp), ("dbias", _vp), ("workspace", _vp),
                ("workspace_bytes", _i64), ("lddy", _i64), ("ldx", _i64), ("lddw", _i64),
                ("M", _i32), ("N", _i32), ("K", _i32), ("dtype", _i32), ("accumulate", _i32),
                ("conv", _i32), ("nb", _i32), ("H", _i32), ("W", _i32), ("Cin", _i32), ("Ho", _i32), ("Wo", _i32),
                ("dy_rows_in", _i32), ("dy_rows_out", _i32), ("dy_row_off", _i32),
                ("x_rows_in", _i32), ("x_rows_out", _i32), ("x_row_off", _i32)]


class AdamPackEntry(ctypes.Structure):
    _fields_ = [("p", _vp), ("g", _vp), ("m", _vp), ("v", _vp), ("dst_lin", _vp), ("dst_t", _vp), ("n", _i64), ("N", _i32), ("K", _i32),
                ("blk_start", _i64)]


class BnBwdDesc(ctypes.Structure):
    _fields_ = [("dy", _vp), ("dpool", _vp), ("y", _vp), ("z", _vp * 2), ("mean", _vp * 2), ("rstd", _vp * 2), ("gamma", _vp * 2),
                ("dgamma", _vp * 2), ("dbeta", _vp * 2), ("dz", _vp * 2), ("g_out", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
                ("rows_per_batch", _i64), ("pool_scale", ctypes.c_float), ("M", _i32), ("C", _i32), ("nbranch", _i32), ("dtype", _i32)]


class RaggedSrc(ctypes.Structure):
    _fields_ = [("f32", _vp), ("u8", _vp), ("H", _i32), ("W", _i32)]


class CpPair(ctypes.Structure):
    _fields_ = [("l_image", _vp), ("l_masks", _vp), ("l_boxes", _vp), ("u_image", _vp), ("u_masks", _vp), ("out_image", _vp), ("out_masks", _vp),
                ("word_off", _i64), ("inter_off", _i64), ("row_off", _i64), ("choice_off", _i64),
                ("Hl", _i32), ("Wl", _i32), ("Nl", _i32), ("Hu", _i32), ("Wu", _i32), ("Nu", _i32), ("nc", _i32), ("h_new", _i32), ("w_new", _i32),
                ("h_shift", _i32), ("w_shift", _i32), ("rh", ctypes.c_float), ("rw", ctypes.c_float), ("sx", ctypes.c_float), ("sy", ctypes.c_float),
                ("reserved", _i32)]


class MlImage(ctypes.Structure):
    _fields_ = [("masks", _vp), ("boxes", _vp), ("index", _vp), ("H", _i32), ("W", _i32), ("G", _i32), ("first", _i32), ("R", _i32),
                ("index64", _i32)]


class BlImage(ctypes.Structure):
    _fields_ = [("boxes", _vp), ("gt_boxes", _vp), ("gt_classes", _vp), ("gt_scores", _vp), ("first", _i32), ("R", _i32), ("G", _i32),
                ("chunk_first", _i32), ("height", ctypes.c_float), ("width", ctypes.c_float)]


class DpImage(ctypes.Structure):
    _fields_ = [("boxes", _vp), ("scores", _vp), ("mat_first", _i64), ("R", _i32), ("cand_first", _i32), ("out_first", _i32), ("cap", _i32),
                ("height", ctypes.c_float), ("width", ctypes.c_float)]


class PermEntry(ctypes.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("d", _i32 * 4), ("sstride", _i64 * 4), ("soff", _i64), ("dtype_in", _i32), ("dtype_out", _i32),
                ("blk_start", _i64), ("e", _i32 * 4), ("ord", _i32 * 4), ("rowlen", _i64)]


# the header's structs and their mirrors above: tests/test_abi_cpu.py compares every size and offset with what a C compiler gives
MIRRORS = {"umr_gemm_desc": GemmDesc, "umr_gemm_tn_desc": GemmTnDesc, "umr_adam_pack_entry": AdamPackEntry, "umr_bn_bwd_desc": BnBwdDesc,
           "umr_ragged_src": RaggedSrc, "umr_cp_pair": CpPair, "umr_ml_image": MlImage, "umr_bl_image": BlImage, "umr_dp_image": DpImage,
           "umr_perm_entry": PermEntry}


def build(verbose=False, jobs=8):
    """Compile every HIP source for gfx950 into unmore_amd/lib/libumr.so (hipcc
    cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, f"-j{jobs}"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-8000:])
    if r.returncode != 0:
        raise RuntimeError("building libumr.so failed")
    return LIB_PATH


_lib = None
_count = [0]     # launches checked so far (graphs.StagedCaptured skips graph segments that recorded nothing)

_ARG = {"int": _i32, "int32_t": _i32, "int64_t": _i64, "float": ctypes.c_float, "double": ctypes.c_double, "umr_stream_t": _vp,
        "const char*": ctypes.c_char_p, "int*": ctypes.POINTER(ctypes.c_int)}     # every other pointer: c_void_p
_RET = {"int": None, "int64_t": _i64, "const char*": ctypes.c_char_p}            # None: ctypes' default, a C int


def _ctype(decl, table, proto):
    c = re.sub(r"\s*\*\s*", "*", " ".join(decl.split()))
    if c not in table and not (table is _ARG and c.endswith("*")):
        raise RuntimeError(f"{HEADER}: no ctypes type for '{c}' in '{' '.join(proto.split())}'")
    return table.get(c, _vp)


def _read_header():
    """The prototypes of include/umr.h as ({name: argtypes}, {name: restype, where it is not int}).  The header is the one description
    of the boundary: a declaration this reader does not understand raises here, at import, instead of being bound by a guess."""
    if not os.path.exists(HEADER):
        raise RuntimeError(f"{HEADER} is missing: the ctypes binding of libumr.so is read from it")
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    args, rets = {}, {}
    for proto in text.split(";"):
        if "(" not in proto:
            continue                                         # enums, the stream typedef, the extern "C" braces
        m = re.fullmatch(r"\s*(.*?)\b(umr_\w+)\s*\(([^()]*)\)\s*", proto, flags=re.S)
        if m is None:
            raise RuntimeError(f"{HEADER}: not a prototype this binding can read: '{' '.join(proto.split())}'")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        args[name] = [_ctype(re.sub(r"\w+\s*$", "", p), _ARG, proto) for p in params]       # a parameter is its type, then its name
        rets[name] = _ctype(ret, _RET, proto)
    return args, {name: r for name, r in rets.items() if r is not None}


ARGTYPES, RESTYPES = _read_header()


def exported_symbols():
    return sorted(ARGTYPES)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the product has no CPU fallback)")
        _lib = ctypes.CDLL(LIB_PATH)
        for name, argtypes in ARGTYPES.items():
            fn = getattr(_lib, name)
            fn.argtypes = argtypes
            if name in RESTYPES:
                fn.restype = RESTYPES[name]
    return _lib


def check(status, what):
    _count[0] += 1
    if status != 0:
        raise RuntimeError(f"{what} failed with status {status}: {lib().umr_last_error_string().decode()}")
