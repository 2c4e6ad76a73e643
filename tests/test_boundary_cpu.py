"""CPU-side checks of the drop-in boundary: the shared library loads and exports exactly the
symbols include/zira_msda.h declares, the `_C` drop-in reproduces the reference's error
behaviour for CPU tensors, and host-side planning helpers answer without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from ziragroundingdino_amd import _C, _header, _lib
from ziragroundingdino_amd import build as zbuild


def header_symbols():
    text = open(os.path.join(ROOT, "include", "zira_msda.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(zira_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    zbuild.build_extension()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = header_symbols()
    assert declared, "no declarations parsed from include/zira_msda.h"
    for sym in declared:
        assert hasattr(lib, sym), "libzira_msda.so does not export %s" % sym
    assert sorted(_lib.SYMBOLS) == declared      # the binding knows exactly the header's surface


def test_every_declaration_is_typed_from_the_header():
    """One prototype of each kind of type, pinned literally; the count against the independent reading above."""
    vp, i, f32, f64, ll, sz = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong,
                               ctypes.c_size_t)
    P = _lib.PROTOTYPES
    assert len(P) == len(header_symbols()) == 100 and tuple(P) == _lib.SYMBOLS
    assert P["zira_msda_fwd_f32"] == (i, [vp] * 5 + [i] * 7 + [vp] * 2)
    assert P["zira_attn_fwd_f32"] == (i, [vp] * 4 + [i] * 8 + [f32, vp, vp, vp]) and P["zira_attn_fwd_f32"][1][12] is f32
    assert P["zira_cat_logits_fwd_f32"] == (i, [vp, vp, vp, vp, ll, i, i, i, i, i, f32, vp, vp, vp])
    assert P["zira_clip_adamw_f32"] == (i, [vp, vp, vp, ctypes.c_int64, vp, i, vp, vp, i] + [f64] * 8 + [i, vp, vp, sz, vp])
    assert P["zira_rsb_workspace_floats"] == (sz, [sz])
    assert P["zira_rsb_fwd_f32"] == (i, [vp, vp, vp, sz, vp, vp, vp, vp])
    assert P["zira_layernorm_fwd_f32"][1][3] is ctypes.c_int64
    assert P["zira_rowgemm_f32"] == (i, [ctypes.POINTER(_lib.RowGemmArgs), vp])
    assert P["zira_place_batch_u8"][1][0] is ctypes.POINTER(_lib.PlaceImage)
    assert P["zira_resample_ws_bytes"] == (sz, [ctypes.POINTER(_lib.ResampleImage), i])
    # the two segment tables are device tensors passed as data_ptr(): an address, which POINTER(struct) would refuse
    assert P["zira_ema_swap_f32"] == (i, [vp, ctypes.c_int64, vp, i, vp, vp])
    assert P["zira_msda_version"] == (ctypes.c_char_p, []) and P["zira_msda_variant_f32"] == (ctypes.c_char_p, [i])
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


STRUCTS = {       # name: (sizeof, [(field, offset, size)])
    "zira_rowgemm_args": (216, [
        ("a", 0, 8), ("lda", 8, 4), ("pos", 16, 8), ("ldpos", 24, 4), ("pos_cols", 28, 4), ("w", 32, 8), ("ldw", 40, 4),
        ("w_is_nk", 44, 4), ("bias", 48, 8), ("res", 56, 8), ("ldres", 64, 4), ("mask", 72, 8), ("relu", 80, 4),
        ("ln_gamma", 88, 8), ("ln_beta", 96, 8), ("ln_eps", 104, 4), ("ln_sum", 112, 8), ("ln_mean", 120, 8),
        ("ln_rstd", 128, 8), ("lnb_x", 136, 8), ("lnb_gamma", 144, 8), ("lnb_mean", 152, 8), ("lnb_rstd", 160, 8),
        ("lnb_dx", 168, 8), ("c", 176, 8), ("ldc", 184, 4), ("m", 188, 4), ("n", 192, 4), ("k", 196, 4), ("batch", 200, 4),
        ("a_batch_first", 204, 4), ("c_batch_first", 208, 4)]),
    "zira_optim_segment": (32, [("param", 0, 8), ("start", 8, 8), ("numel", 16, 8), ("group", 24, 8)]),
    "zira_place_image": (32, [("data", 0, 8), ("h", 8, 4), ("w", 12, 4), ("stride_c", 16, 8), ("stride_r", 24, 8)]),
    "zira_resample_image": (64, [("src", 0, 8), ("dst", 8, 8), ("stride_c", 16, 8), ("stride_r", 24, 8), ("stride_x", 32, 8),
                                 ("h", 40, 4), ("w", 44, 4), ("new_h", 48, 4), ("new_w", 52, 4), ("flip", 56, 4)]),
    "zira_ema_segment": (24, [("param", 0, 8), ("start", 8, 8), ("numel", 16, 8)]),
}


def test_structs_are_laid_out_as_the_compiler_lays_them_out():
    """sizeof / offsetof as a host C compiler gives them for the header (x86-64)."""
    assert list(_lib.STRUCTS) == list(STRUCTS)
    for name, (size, fields) in STRUCTS.items():
        cls = _lib.STRUCTS[name]
        assert ctypes.sizeof(cls) == size, name
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == fields, name
    assert _lib.RowGemmArgs is _lib.STRUCTS["zira_rowgemm_args"] and _lib.PlaceImage is _lib.STRUCTS["zira_place_image"]
    assert _lib.ResampleImage is _lib.STRUCTS["zira_resample_image"]
    assert _lib.RowGemmArgs._fields_[15] == ("ln_eps", ctypes.c_float) and _lib.PlaceImage._fields_[1] == ("h", ctypes.c_int32)
    assert _lib.ResampleImage._fields_[2] == ("stride_c", ctypes.c_int64)


def test_limits_are_the_header_s():
    assert _lib.CONSTANTS == {
        "ZIRA_MSDA_EINVAL": 1, "ZIRA_OPTIM_TAIL_CHUNK": 4096, "ZIRA_OPTIM_TAIL_MAX_GROUPS": 8, "ZIRA_PLACE_MAX_IMAGES": 8,
        "ZIRA_AP_MAX_THRS": 16, "ZIRA_AP_MAX_AREAS": 4, "ZIRA_AP_MAX_DETS": 8, "ZIRA_AP_MAX_RECS": 256,
        "ZIRA_AP_MAX_CLASSES": 65535, "ZIRA_VOC_MAX_THRS": 16, "ZIRA_RESAMPLE_MAX_IMAGES": 8, "ZIRA_RESAMPLE_MAX_SIDE": 4096,
        "ZIRA_RESAMPLE_MAX_TAPS": 17, "ZIRA_EMA_CHUNK": 4096, "ZIRA_EMA_MAX_N": 1 << 31}
    assert (_lib.PLACE_MAX_IMAGES, _lib.AP_MAX_THRS, _lib.AP_MAX_AREAS, _lib.VOC_MAX_THRS) == (8, 16, 4, 16)
    assert (_lib.AP_MAX_DETS, _lib.AP_MAX_RECS, _lib.AP_MAX_CLASSES) == (8, 256, 65535)
    assert (_lib.RESAMPLE_MAX_IMAGES, _lib.RESAMPLE_MAX_SIDE, _lib.RESAMPLE_MAX_TAPS) == (8, 4096, 17)
    from ziragroundingdino_amd import ema, optim_tail          # their import also asserts the segment rows' layout

    assert (ema.CHUNK, ema.MAX_N, optim_tail.CHUNK, optim_tail.MAX_GROUPS) == (4096, 1 << 31, 4096, 8)


def test_segment_rows_must_match_the_struct():
    _lib.assert_int64_rows(_lib.EmaSegment, ("param", "start", "numel"))
    for names in (("param", "numel", "start"), ("param", "start"), ("param", "start", "numel", "group")):
        with pytest.raises(AssertionError):
            _lib.assert_int64_rows(_lib.EmaSegment, names)
    with pytest.raises(AssertionError):
        _lib.assert_int64_rows(_lib.PlaceImage, ("data", "h", "w", "stride_c", "stride_r"))      # 4-byte members


@pytest.mark.parametrize("text, named", [
    ("int zira_ok(int a);\n\nint zira_f(const float *x,\n    unsigned n, void *stream);\n", r"line 3.*unsigned n"),
    ("typedef struct zira_s {\n    int a, b;\n    short c;\n} zira_s;\n", r"line 3.*short c"),
    ("/* two\n lines */\nint zira_g(const zira_nope *p, void *stream);\n", r"line 3.*zira_nope \*p"),
    ("typedef struct zira_s { int a; } zira_s;\nint zira_h(zira_s by_value);\n", r"line 2.*zira_s by_value"),
    ("#define ZIRA_SHIFTED (1 << 4)\n", r"line 1.*ZIRA_SHIFTED"),
    ("long zira_k(void);\n", r"line 1.*long zira_k"),
    ("int zira_a(int a);\nstatic inline int helper(int a) { return a; }\n", r"line 2"),
])
def test_the_reader_refuses_what_it_cannot_map(tmp_path, text, named):
    path = tmp_path / "bad.h"
    path.write_text(text)
    with pytest.raises(_header.HeaderError, match=named):
        _header.parse(path.read_text())


def test_the_reader_on_a_small_header():
    protos, structs, consts = _header.parse(
        "#ifndef ZIRA_T_H_\n#define ZIRA_T_H_\n#define ZIRA_T_MAX 0x10u // hex\n#define ZIRA_T_BIG 4294967296ll\n"
        "typedef struct zira_t { const void *p; int32_t h, w; int64_t s; float f; } zira_t;\n"
        "typedef struct zira_d { void *p; } zira_d;\n"
        "size_t zira_t_bytes(const zira_t *t, const zira_d *d, long long n,\n   unsigned char *m);\n"
        "const char *zira_t_name();\n#endif\n", device_tables=("zira_d",))
    assert consts == {"ZIRA_T_MAX": 16, "ZIRA_T_BIG": 1 << 32}
    assert structs["zira_t"]._fields_ == [("p", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                                          ("s", ctypes.c_int64), ("f", ctypes.c_float)]
    assert protos == {"zira_t_bytes": (ctypes.c_size_t, [ctypes.POINTER(structs["zira_t"]), ctypes.c_void_p,
                                                         ctypes.c_longlong, ctypes.c_void_p]),
                      "zira_t_name": (ctypes.c_char_p, [])}


def test_missing_header_fails_loudly(tmp_path):
    with pytest.raises(ImportError, match="cannot read .*nope.h"):
        _lib.read_header(str(tmp_path / "nope.h"))


def test_host_only_entry_points_work_without_gpu():
    lib = _lib.load()
    assert _lib.version().startswith("zira_msda")
    assert _lib.variant_f32(32) and _lib.variant_f32(24) == "generic"
    # north-star decoder shape: the atomic-free backward applies and needs a few MB of scratch
    n = lib.zira_msda_bwd_workspace_bytes(2, 22223, 8, 32, 4, 900, 4)
    assert 1 << 20 < n < 1 << 28
    assert lib.zira_msda_bwd_workspace_bytes(2, 22223, 8, 24, 4, 900, 4) == 0   # D=24: generic path only
    assert lib.zira_msda_bwd_workspace_bytes(0, 1, 1, 32, 1, 1, 1) == 0
    assert lib.zira_rsb_workspace_floats(1 << 20) > 0
    # argument errors are reported, never thrown, and nothing is launched
    assert lib.zira_msda_fwd_f32(None, None, None, None, None, 1, 1, 1, 32, 1, 1, 1, None, None) == 1


def test_workspace_sizes_at_the_model_shapes():
    """The scratch the model's two MSDA backward calls ask for, pinned: encoder (Q = S, the cell kernels; no plan) and
    decoder (Q = 900, plan + tile accumulate; the workspace is the plan buffer).  The plan layout reads the device's CU
    count; without a GPU it assumes 256, which is also the MI355X's, so the same values hold on both machines."""
    lib = _lib.load()
    enc, dec = (2, 22223, 8, 32, 4, 22223, 4), (2, 22223, 8, 32, 4, 900, 4)
    assert lib.zira_msda_bwd_workspace_bytes(*enc) == 495588096
    assert lib.zira_msda_plan_bytes(*enc) == 0
    assert lib.zira_msda_bwd_workspace_bytes(*dec) == 123377408
    assert lib.zira_msda_plan_bytes(*dec) == 123377408


def test_cpu_tensors_raise_like_the_reference():
    v = torch.zeros(1, 4, 2, 32)
    sh = torch.tensor([[2, 2]])
    st = torch.tensor([0])
    loc = torch.zeros(1, 3, 2, 1, 4, 2)
    attn = torch.zeros(1, 3, 2, 1, 4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _C.ms_deform_attn_forward(v, sh, st, loc, attn, 64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _C.ms_deform_attn_backward(v, sh, st, loc, attn, torch.zeros(1, 3, 64), 64)


def test_missing_extension_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError, match="no CPU fallback"):
        _lib.load()
