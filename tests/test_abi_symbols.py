"""CPU checks of the C-ABI boundary: the library builds in-tree, loads, and exports every
entry point include/radmmm_hip.h declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "radmmm_hip.h")
LIB = os.path.join(ROOT, "rad_mmm_amd", "libradmmm_hip.so")


def declared_functions():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(radmmm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_path():
    names = declared_functions()
    for must in ("radmmm_rowgemm_f32", "radmmm_wgrad_f32", "radmmm_weightnorm_fwd", "radmmm_weightnorm_bwd",
                 "radmmm_affine_coupling_fwd", "radmmm_affine_coupling_bwd", "radmmm_masked_reduce",
                 "radmmm_pq_spline_fwd", "radmmm_pq_spline_bwd", "radmmm_attn_fwd", "radmmm_attn_bwd",
                 "radmmm_mas_width1", "radmmm_stft_mel", "radmmm_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(LIB)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing
    lib.radmmm_abi_version.restype = ctypes.c_int
    import re
    hdr = open(os.path.join(ROOT, "include", "radmmm_hip.h")).read()
    assert lib.radmmm_abi_version() == int(re.search(r"#define RADMMM_ABI_VERSION (\d+)", hdr).group(1)) >= 2
    lib.radmmm_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.radmmm_last_error(), bytes)


def test_argument_validation_without_gpu():
    """Descriptor validation happens before any HIP call, so it is testable on CPU."""
    lib = ctypes.CDLL(LIB)
    lib.radmmm_last_error.restype = ctypes.c_char_p
    assert lib.radmmm_rowgemm_f32(None, None) == -1
    assert b"null descriptor" in lib.radmmm_last_error()
    assert lib.radmmm_wgrad_f32(None, None) == -1


def test_lstm_entry_points_validate_without_gpu():
    """radmmm_lstm_fwd / radmmm_lstm_bwd refuse null pointers and H = 769 (one past the largest size class) with -1 before
    any HIP call: the null check comes first, so the dims case passes dummy non-null addresses, which that path never
    dereferences.  The path query reports 0 on a thread that has not run a recurrence."""
    lib = ctypes.CDLL(LIB)
    lib.radmmm_last_error.restype = ctypes.c_char_p
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.radmmm_lstm_fwd.argtypes = [p] * 8 + [i, i, i, p]
    lib.radmmm_lstm_bwd.argtypes = [p] * 8 + [i, i, i, p, p]
    lib.radmmm_lstm_last_path.argtypes = [i]
    d = 0x1000                                                   # never dereferenced
    assert lib.radmmm_lstm_fwd(None, d, d, d, None, d, d, None, 2, 3, 8, None) == -1
    assert b"lstm_fwd: null pointer" in lib.radmmm_last_error()
    assert lib.radmmm_lstm_bwd(d, d, None, d, None, d, d, d, 2, 3, 8, None, None) == -1
    assert b"lstm_bwd: null pointer" in lib.radmmm_last_error()
    for H in (769, 0, -8):
        assert lib.radmmm_lstm_fwd(d, d, d, d, None, d, d, None, 2, 3, H, None) == -1
        assert b"lstm_fwd: bad dims" in lib.radmmm_last_error()
        assert lib.radmmm_lstm_bwd(d, d, d, d, None, d, d, d, 2, 3, H, None, None) == -1
        assert b"lstm_bwd: bad dims" in lib.radmmm_last_error()
    for B, T in ((0, 3), (2, 0)):
        assert lib.radmmm_lstm_fwd(d, d, d, d, None, d, d, None, B, T, 8, None) == -1
        assert lib.radmmm_lstm_bwd(d, d, d, d, None, d, d, d, B, T, 8, None, None) == -1
    assert [lib.radmmm_lstm_last_path(w) for w in (0, 1, 2, -1)] == [0, 0, 0, 0]


def test_rowgemm_h3_kernel_query_without_gpu():
    """radmmm_rowgemm_h3_last_kernel is thread-local and reports 0 until a launch decision was made on the calling thread:
    a refused descriptor (validation comes before any HIP call) leaves it alone.  The code's fields are the header's macro."""
    import threading
    import rad_mmm_amd._lib as L
    lib = ctypes.CDLL(LIB)
    lib.radmmm_last_error.restype = ctypes.c_char_p
    lib.radmmm_rowgemm_h3_last_kernel.restype = ctypes.c_int
    seen = []

    def fresh_thread():
        seen.append(lib.radmmm_rowgemm_h3_last_kernel())
        seen.append(lib.radmmm_rowgemm_h3(None, None))
        seen.append(lib.radmmm_last_error())
        d = L.RowGemmH3Desc()                                     # null operands: refused before any kernel is chosen
        seen.append(lib.radmmm_rowgemm_h3(ctypes.byref(d), None))
        seen.append(lib.radmmm_rowgemm_h3_last_kernel())

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert seen[0] == 0 and seen[1] == -1 and b"null descriptor" in seen[2] and seen[3] == -1 and seen[4] == 0
    hdr = open(HDR).read()
    assert "#define RADMMM_H3_KERNEL_CODE(family, nprod, mb, ek) ((family) * 1000 + (nprod) * 100 + (mb) * 10 + (ek))" in hdr
    for name, val in (("NARROW", L.H3_NARROW), ("H3D", L.H3_H3D), ("WIN", L.H3_WIN), ("ONE", L.H3_ONE)):
        assert re.search(rf"#define RADMMM_H3_FAMILY_{name} {val}\b", hdr)
    assert L.h3_kernel_code(L.H3_WIN, 2, 7, L.EK_DGRAD) == 3274


def test_h3_plan_query_without_gpu(monkeypatch):
    """radmmm_rowgemm_h3_plan shares the entry point's validation and decision: a null or a refused descriptor gives the entry
    point's code and error text, an accepted one the header's kernel code.  Only refused descriptors go to the entry point
    itself: an accepted one would launch on the stand-in addresses where there is a GPU."""
    import pytest
    import rad_mmm_amd._lib as L
    lib = L.lib
    for k in ("RADMMM_H3_TILE", "RADMMM_H3W_MB", "RADMMM_SLOT3", "RADMMM_WIN", "RADMMM_ONE", "RADMMM_WIN_XT"):
        monkeypatch.delenv(k, raising=False)
    assert lib.radmmm_rowgemm_h3_plan(None) == -1 and lib.radmmm_last_error() == b"rowgemm_h3: null descriptor"
    assert lib.radmmm_rowgemm_h3(None, None) == -1 and lib.radmmm_last_error() == b"rowgemm_h3: null descriptor"
    a = 0x10000                                                  # never dereferenced
    ok = dict(Ah=a, Al=a, Bh=a, Bl=a, C=a, lda_h=64, ldb_h=64, b_tap_stride_h=64 * 512, ldc=512, M=4096, N=512, K=64, T=512)
    refused = [(dict(ok, Al=None), b"rowgemm_h3: null operand"),
               (dict(ok, K=48), b"rowgemm_h3: K=48 must be a multiple of 32"),
               (dict(ok, b_layout=1), b"rowgemm_h3: both operands are K-contiguous"),
               (dict(ok, sign=0), b"rowgemm_h3: sign must be +-1"),
               (dict(ok, nprod=2, lda_h=72), b"rowgemm_h3: nprod 2 needs ld % 32 == 0")]
    for kw, text in refused:
        d = L._h3_desc(kw, L._addr)
        assert lib.radmmm_rowgemm_h3_plan(ctypes.byref(d)) == -1 and lib.radmmm_last_error().startswith(text)
        mine = lib.radmmm_last_error()
        assert lib.radmmm_rowgemm_h3(ctypes.byref(d), None) == -1 and lib.radmmm_last_error() == mine
        assert lib.radmmm_rowgemm_h3_colsum_rows(ctypes.byref(L._h3_desc(dict(kw, colsum_scratch=a), L._addr))) == 0
    with pytest.raises(L.RadmmmError, match="null operand"):
        L.rowgemm_h3_plan(**dict(ok, Al=None))
    # 8 x 2 tiles of 128 x 256 are fewer than 128 workgroups: the narrow kernel; 128 x 2 are not: the wide tiles (their
    # height pinned here: the cost model's choice follows the CU count)
    assert L.rowgemm_h3_plan(**dict(ok, M=1024)) == L.h3_kernel_code(L.H3_NARROW, 3, 4, 0)
    monkeypatch.setenv("RADMMM_H3W_MB", "7")
    wide = dict(ok, M=16384, nprod=2)
    assert L.rowgemm_h3_plan(**dict(wide, taps=5)) == L.h3_kernel_code(L.H3_WIN, 2, 7, L.EK_PLAIN)
    assert L.rowgemm_h3_plan(**wide) == L.h3_kernel_code(L.H3_ONE, 2, 7, L.EK_PLAIN)
    assert lib.radmmm_rowgemm_h3_colsum_rows(ctypes.byref(L._h3_desc(dict(wide, colsum_scratch=a), L._addr))) == (16384 + 223) // 224
    assert "int radmmm_rowgemm_h3_plan(const radmmm_rowgemm_h3_desc* d);" in open(HDR).read()


def test_f32_plan_queries_without_gpu():
    """radmmm_rowgemm_f32_plan / radmmm_wgrad_f32_plan make no HIP call and share the entry points' validation: a null or a
    refused descriptor gives the entry point's code and error text, an accepted one the header's kernel code."""
    import pytest
    import rad_mmm_amd._lib as L
    lib = L.lib
    for plan, entry, what in ((lib.radmmm_rowgemm_f32_plan, lib.radmmm_rowgemm_f32, b"rowgemm"), (lib.radmmm_wgrad_f32_plan, lib.radmmm_wgrad_f32, b"wgrad")):
        assert plan(None) == -1
        assert lib.radmmm_last_error() == what + b": null descriptor"
        assert entry(None, None) == -1 and lib.radmmm_last_error() == what + b": null descriptor"
    a = 0x10000                                                  # never dereferenced
    refused = [(L._rowgemm_desc({}, L._addr), b"rowgemm: null operand"),
               (L._rowgemm_desc(dict(A=a, B=a, C=a, lda=16, ldb=16, ldc=8, M=10, N=8, K=16, T=3), L._addr), b"rowgemm: M=10 is not a multiple of T=3"),
               (L._rowgemm_desc(dict(A=a + 4, B=a, C=a, lda=16, ldb=16, ldc=8, M=9, N=8, K=16, T=3), L._addr), b"rowgemm: A must be 16B aligned"),
               (L._rowgemm_desc(dict(A=a, B=a, C=a, lda=16, ldb=16, ldc=8, M=9, N=8, K=16, T=3, sign=0), L._addr), b"rowgemm: sign must be +-1"),
               (L._rowgemm_desc(dict(A=a, B=a, C=a, lda=16, ldb=16, ldc=8, M=9, N=8, K=16, T=3, dact=2), L._addr), b"rowgemm: dact needs dact_src")]
    for d, text in refused:
        assert lib.radmmm_rowgemm_f32_plan(ctypes.byref(d)) == -1 and lib.radmmm_last_error().startswith(text)
        mine = lib.radmmm_last_error()
        assert lib.radmmm_rowgemm_f32(ctypes.byref(d), None) == -1 and lib.radmmm_last_error() == mine
    for kw, text in ((dict(), b"wgrad: null operand"), (dict(GY=a, X=a, P=a, ldgy=16, ldx=16, ldp=16, R=10, Mc=8, Nc=8, T=3), b"wgrad: R=10 is not a multiple of T=3"),
                     (dict(GY=a, X=a, P=a, ldgy=16, ldx=16, ldp=7, R=9, Mc=8, Nc=8, T=3), b"wgrad: ldp < Nc")):
        d = L._wgrad_desc(kw, L._addr)
        assert lib.radmmm_wgrad_f32_plan(ctypes.byref(d)) == -1 and lib.radmmm_last_error().startswith(text)
        mine = lib.radmmm_last_error()
        assert lib.radmmm_wgrad_f32(ctypes.byref(d), None) == -1 and lib.radmmm_last_error() == mine
    with pytest.raises(L.RadmmmError, match="not a multiple"):
        L.rowgemm_plan(A=a, B=a, C=a, lda=16, ldb=16, ldc=8, M=10, N=8, K=16, T=3)
    assert L.rowgemm_plan(A=a, B=a, C=a, lda=16, ldb=16, ldc=8, M=9, N=8, K=16, T=3) == L.f32_kernel_code(L.F32_ROWS16, 0, 4, 9)
    assert L.rowgemm_plan(A=a, B=a, C=a, lda=16, ldb=8, ldc=8, M=9, N=8, K=6, T=3, b_layout=1) == L.f32_kernel_code(L.F32_GENERIC, 1)
    assert L.rowgemm_plan(A=a, B=a, C=a, lda=160, ldb=160, ldc=160, M=9, N=160, K=160, T=3) == L.f32_kernel_code(L.F32_MIX)
    assert L.wgrad_plan(GY=a, X=a, P=a, ldgy=8, ldx=8, ldp=8, R=32, Mc=8, Nc=8, T=16) == L.f32_kernel_code(L.F32_WGRAD16)
    assert L.wgrad_plan(GY=a, X=a, P=a, ldgy=8, ldx=8, ldp=8, R=30, Mc=8, Nc=8, T=15) == L.f32_kernel_code(L.F32_WGRAD)
    hdr = open(HDR).read()
    assert "#define RADMMM_F32_KERNEL_CODE(family, bl, mt, rows) ((family) * 1000000 + (bl) * 100000 + (mt) * 1000 + (rows))" in hdr
    for name, val in (("GENERIC", L.F32_GENERIC), ("ROWS16", L.F32_ROWS16), ("MIX", L.F32_MIX), ("WGRAD", L.F32_WGRAD), ("WGRAD16", L.F32_WGRAD16)):
        assert re.search(rf"#define RADMMM_F32_FAMILY_{name}\s+{val}\b", hdr)
    assert L.f32_kernel_code(L.F32_ROWS16, 1, 13, 193) == 2113193


def test_python_binding_matches_struct_layout():
    import rad_mmm_amd._lib as L
    # field order/size of the ctypes mirrors == the C structs (checked via a tiny C probe is not
    # possible without hipcc at test time; check the sizes the compiler is known to produce)
    assert ctypes.sizeof(L.RowGemmDesc) % 8 == 0 and ctypes.sizeof(L.WgradDesc) % 8 == 0
    assert L.RowGemmDesc.a_item_stride.offset == 16 and L.RowGemmDesc.B.offset == 24


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "rad_mmm_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("# oracle", ""), fn
    bench = open(os.path.join(ROOT, "bench.py")).read() if os.path.exists(os.path.join(ROOT, "bench.py")) else ""
    assert "rad_mmm_amd" in bench or bench == ""


def test_header_is_plain_c():
    """The boundary is a C ABI: the header must compile as C99 on its own."""
    import subprocess
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HDR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ctypes_structs_match_the_c_layout(tmp_path):
    """sizeof / offsetof of every descriptor field as gcc lays the header's structs out == the ctypes mirrors."""
    import subprocess
    import rad_mmm_amd._lib as L
    pairs = [("radmmm_rowgemm_desc", L.RowGemmDesc), ("radmmm_wgrad_desc", L.WgradDesc),
             ("radmmm_rowgemm_h3_desc", L.RowGemmH3Desc), ("radmmm_wn_item", L.WnItem), ("radmmm_tp_item", L.TpItem), ("radmmm_cs_item", L.CsItem), ("radmmm_dact_item", L.DactItem)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void) {"]
    for cname, mirror in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, mirror in pairs:
        assert int(got[cname]) == ctypes.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, f"{cname}.{fname}"


def test_ctypes_signatures_have_the_declared_arity():
    """Every function's ctypes argtypes list is as long as its parameter list in the header."""
    import rad_mmm_amd._lib as L
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    protos = dict(re.findall(r"\b(radmmm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))
    checked = 0
    for name, params in protos.items():
        fn = getattr(L.lib, name)
        if fn.argtypes is None:
            continue
        params = params.strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert len(fn.argtypes) == n, (name, len(fn.argtypes), n)
        checked += 1
    assert checked >= 40


def test_ctypes_signatures_have_the_declared_types():
    """Per parameter: pointer / int / int64 / float / double class of the header == the ctypes argtype."""
    import rad_mmm_amd._lib as L
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    protos = dict(re.findall(r"\b(radmmm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))

    def c_class(p):
        p = " ".join(p.split())
        if "*" in p or "radmmm_stream_t" in p:
            return "ptr"
        for key, cls in (("int64_t", "i64"), ("double", "f64"), ("float", "f32"), ("int32_t", "i32"), ("int", "i32")):
            if re.search(rf"\b{key}\b", p):
                return cls
        raise AssertionError(f"unclassified parameter {p!r}")

    def py_class(t):
        if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
            return "ptr"
        return {ctypes.c_int: "i32", ctypes.c_int64: "i64", ctypes.c_longlong: "i64", ctypes.c_float: "f32",
                ctypes.c_double: "f64"}[t]

    for name, params in protos.items():
        fn = getattr(L.lib, name)
        if fn.argtypes is None or params.strip() in ("", "void"):
            continue
        want = [c_class(p) for p in params.split(",")]
        got = [py_class(t) for t in fn.argtypes]
        assert want == got, (name, want, got)


def test_grad_scale_state_survives_module_copies():
    """ops.GradScale holds a CUDA event and pinned memory once used: deep copies / pickles of the owning module must get a
    fresh state instead of failing (EMA copies, torch.save(model))."""
    import copy
    import pickle
    from rad_mmm_amd import ops
    gs = ops.GradScale()
    gs.S = 4.0
    assert copy.deepcopy(gs).S is None
    assert pickle.loads(pickle.dumps(gs)).S is None
    assert gs.get("S") == 4.0 and gs.get("other", 7) == 7
