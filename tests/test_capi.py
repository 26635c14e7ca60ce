"""CPU: the C-ABI shared library builds/loads and exports exactly what include/hoisdf.h declares, and the ctypes binding that
hoisdf_amd/_lib.py derives from the header agrees with it: argument counts by an independent count, every struct's size and every
field's offset and size by the host C compiler.  No compute calls here (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from hoisdf_amd import _lib

HEADER = open(_lib.HEADER_PATH).read()


def header_functions():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    fns = {}
    for m in re.finditer(r"\b(?:int|long|void|const char\*|const uint32_t\*)\s+(hoisdf_\w+)\s*\(([^;]*?)\)\s*;", body, flags=re.S):
        args = m.group(2).strip()
        n = 0 if args in ("void", "") else len(args.split(","))
        fns[m.group(1)] = n
    return fns


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_header_declares_a_reasonable_surface():
    fns = header_functions()
    assert len(fns) >= 25
    for must in ("hoisdf_project_gather_fwd", "hoisdf_linear_fwd", "hoisdf_attention_fwd", "hoisdf_attention_bwd",
                 "hoisdf_select_smallest_abs", "hoisdf_vote_fwd", "hoisdf_last_error", "hoisdf_version"):
        assert must in fns


def test_library_exports_every_declared_symbol(lib):
    for name in header_functions():
        assert hasattr(lib, name), f"libhoisdf_hip.so does not export {name}"


def test_ctypes_table_matches_header(lib):
    fns = header_functions()
    assert set(fns) == set(_lib.FUNCTIONS) == set(_lib.exported_symbols())
    for name, (args, ret) in _lib.FUNCTIONS.items():
        assert len(args) == fns[name], f"{name}: {len(args)} ctypes args vs {fns[name]} in the header"
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is ret, name
    # the three views split the table: status entries (through `call`), the two argument-less strings, the rest
    assert _lib._STATUS == set(_lib.SIGNATURES) and all(_lib.FUNCTIONS[n][1] is C.c_int for n in _lib.SIGNATURES)
    assert set(_lib._RET) == {"hoisdf_version", "hoisdf_last_error"}
    assert not (set(_lib.SIGNATURES) | set(_lib._RET)) & set(_lib._OTHER)
    assert len(_lib.SIGNATURES) + len(_lib._RET) + len(_lib._OTHER) == len(fns)
    assert "hoisdf_linear_fwd" in _lib.SIGNATURES and "hoisdf_crop_params_ho3d" in _lib.SIGNATURES
    assert _lib._OTHER["hoisdf_linear_emu_pieces"] == ([], C.c_int) and _lib._OTHER["hoisdf_set_gemm_emu"] == ([C.c_int], None)
    assert _lib._OTHER["hoisdf_bn_workspace_floats"] == ([C.c_long, C.c_int], C.c_long)
    assert _lib.FUNCTIONS["hoisdf_adamw_step"][0][2:8] == [C.c_double] * 5 + [C.c_long]


def test_library_exports_exactly_the_parsed_prototypes(lib):
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (hoisdf_\w+)", syms))
    # hoisdf_internal_*: how the plain-C objects of the library reach its thread-local error message; not ABI, not declared
    public = {s for s in exported if not s.startswith("hoisdf_internal_")}
    assert public == set(_lib.FUNCTIONS), public ^ set(_lib.FUNCTIONS)


def test_constants_and_class_names_come_from_the_header():
    for name in ("MAX_LEVELS", "MLP_MAX_LAYERS", "POSE_MAX_LAYERS", "CROP_MAX_POINTS"):
        (value,) = re.findall(rf"^#define HOISDF_{name} (\d+)$", HEADER, flags=re.M)
        assert getattr(_lib, name) == _lib.CONSTANTS[name] == int(value)
    c_names = re.findall(r"\}\s*(hoisdf_\w+)\s*;", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    c_names.remove("hoisdf_status")                                            # the enum
    assert c_names == list(_lib.STRUCTS) and len(c_names) >= 22
    for c_name, cls in _lib.STRUCTS.items():
        assert getattr(_lib, cls.__name__) is cls and cls.__name__.lower() == c_name[len("hoisdf_"):].replace("_", "")
    assert {"SdfWeights", "EmuPrepItem", "Mlp", "PyramidGrad", "AdamwChunk"} <= {c.__name__ for c in _lib.STRUCTS.values()}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof / offsetof from a host-only C program over the header (compiled as csrc/Makefile compiles its plain C) against ctypes"""
    cc = os.environ.get("CC") or next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None or not shutil.which(cc):
        pytest.skip("no host C compiler")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "hoisdf.h"', "int main(void) {"]
    expected = {}
    for c_name, cls in _lib.STRUCTS.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        expected[c_name] = [C.sizeof(cls)]
        for field, _ in cls._fields_:
            lines.append(f'  printf("{c_name}.{field} %zu %zu\\n", offsetof({c_name}, {field}), sizeof((({c_name}*)0)->{field}));')
            expected[f"{c_name}.{field}"] = [getattr(cls, field).offset, getattr(cls, field).size]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([cc, "-O2", "-std=c11", "-Wall", "-I", os.path.dirname(_lib.HEADER_PATH), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    measured = {k: [int(v) for v in rest] for k, *rest in (line.split() for line in out.splitlines())}
    assert len(measured) == len(expected) >= 282                 # 22 structs + 260 fields when this test was written
    for key, want in expected.items():
        assert measured[key] == want, f"{key}: the C compiler says {measured[key]}, ctypes {want}"


_MINI = "#define HOISDF_N 4\ntypedef struct hoisdf_t { const float *a, *b[HOISDF_N + 1]; TYPE n; } hoisdf_t;\n" \
        "PROTO\n"


def test_parser_reads_the_dialect_and_refuses_the_rest():
    consts, structs, fns, status = _lib.parse_header(
        _MINI.replace("TYPE", "int64_t").replace("PROTO", "long hoisdf_f(const hoisdf_t* t, double x /* why */, void* stream);"))
    assert consts == {"N": 4} and [n for n, _ in structs["hoisdf_t"]._fields_] == ["a", "b", "n"] and structs["hoisdf_t"].__name__ == "T"
    assert C.sizeof(structs["hoisdf_t"]) == 8 * 7 and fns == {"hoisdf_f": ([C.c_void_p, C.c_double, C.c_void_p], C.c_long)} and not status
    ok = _MINI.replace("TYPE", "int").replace("PROTO", "int hoisdf_f(int n, void* stream);")
    assert _lib.parse_header(ok)[3] == {"hoisdf_f"}
    for bad, what in ((ok.replace("int n;", "size_t n;"), "size_t"),                      # unknown scalar in a struct
                      (ok.replace("(int n", "(unsigned n"), "unsigned"),                  # ... in a prototype
                      (ok.replace("int hoisdf_f", "hoisdf_status hoisdf_f"), "hoisdf_status"),   # ... as a return type
                      (ok.replace("(int n", "(hoisdf_t t"), "hoisdf_t"),                  # a struct by value
                      (ok.replace("int n;", "int n : 3;"), "n : 3"),                      # a member it cannot split
                      (ok.replace("HOISDF_N + 1", "HOISDF_M"), "HOISDF_M"),               # an unknown bound
                      (ok.replace("void* stream)", "void* stream"), "hoisdf_f"),          # a half-matched prototype
                      (ok.replace("(int n", "(int"), "int"),                              # a nameless parameter
                      (ok + "#pragma pack(1)\n", "pragma"),
                      (ok + "int other_f(void);\n", "other_f")):
        with pytest.raises(_lib.HeaderError, match=re.escape(what)):
            _lib.parse_header(bad)


def test_version_and_error_strings(lib):
    assert b"gfx950" in lib.hoisdf_version()
    assert isinstance(lib.hoisdf_last_error(), bytes)


def test_argument_validation_needs_no_gpu(lib):
    """bad arguments are rejected before any HIP call"""
    rc = lib.hoisdf_linear_fwd(None, 4, None, 4, None, None, 4, 8, 4, 4, 0, 0.0, 0, None, None)
    assert rc == -1 and b"null" in lib.hoisdf_last_error()
    with pytest.raises(_lib.HoisdfError):
        _lib.call("hoisdf_select_smallest_abs", None, None, None, 1, 1, None, None)


def test_no_cpu_fallback():
    import torch
    from hoisdf_amd import ops
    with pytest.raises(RuntimeError):
        ops.linear(torch.zeros(2, 4), torch.zeros(3, 4))


def test_collective_library_exports_its_header():
    """include/hoisdf_collective.h <-> libhoisdf_rccl.so (symbol table only: loading it would pull RCCL in)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "hoisdf_amd", "libhoisdf_rccl.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "hoisdf_collective.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hoisdf_\w+)\s*\(", hdr))
    assert {"hoisdf_allreduce", "hoisdf_coll_init", "hoisdf_coll_unique_id", "hoisdf_coll_destroy"} <= declared
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (hoisdf_\w+)", syms))
    assert declared <= exported, declared - exported


def test_coarse_entries_size_queries_and_validation_need_no_gpu(lib):
    """the module-granularity entries: size queries are pure host arithmetic (the same carving code as the real call, dry), and
    malformed descriptors / null buffers are refused before any launch"""
    import ctypes as C
    d = _lib.EncoderLayerDesc(B=32, S=2048, E=256, F=1024, H=4, n_query=1536, n_inter=1536, eps=1e-5, drop_p=0.1, attention=2,
                              attention_bwd_emulated=1, training=1)
    saved = lib.hoisdf_encoder_layer_saved_bytes(C.addressof(d))
    wf, wb = lib.hoisdf_encoder_layer_workspace_bytes(C.addressof(d), 0), lib.hoisdf_encoder_layer_workspace_bytes(C.addressof(d), 1)
    assert saved > 2048 * 32 * 256 * 4 * 3 and wf > 0 and wb > wf                 # at least the q | k | v projections are kept
    d.E = 250                                                                    # not a multiple of the head count / of 4
    assert lib.hoisdf_encoder_layer_saved_bytes(C.addressof(d)) == -1
    assert lib.hoisdf_encoder_layer_fwd(None, None, C.addressof(d), None, None, None, 0, None, 0, None) == -1
    dd = _lib.DecoderLayerDesc(B=32, Q=17, S=2048, E=256, F=1024, H=4, kv_len=1536, eps=1e-5, drop_p=0.1, training=1)
    assert lib.hoisdf_decoder_layer_saved_bytes(C.addressof(dd)) > 0 and lib.hoisdf_decoder_layer_workspace_bytes(C.addressof(dd), 1) > 0
    dd.Q = 65                                                                    # the masked self-attention kernel holds <= 64 queries
    assert lib.hoisdf_decoder_layer_saved_bytes(C.addressof(dd)) == -1
    assert lib.hoisdf_sdf_query_train_saved_bytes(49152, 992) > 49152 * 992 * 4 and lib.hoisdf_sdf_query_train_workspace_bytes(49152, 992, 1) > 0
    assert lib.hoisdf_sdf_infer_workspace(100000, 32, 992) > 0 and lib.hoisdf_sdf_infer_workspace(-1, 32, 992) == -1
    assert lib.hoisdf_mano_dirs_image_floats() == 145 * 2334 + 16 * 778
    assert lib.hoisdf_mano_head_fwd(None, 96, 0, None, 10, 4, None, None, None, None, None, None, None, None, None, 0, 0, None, None, None,
                                    None, None) == -1 and b"null" in lib.hoisdf_last_error()
    assert lib.hoisdf_mano_head_fwd(None, 96, 0, None, 10, 0, None, None, None, None, None, None, None, None, None, 0, 0, None, None, None,
                                    None, None) == 0                                # zero hands: nothing to do
