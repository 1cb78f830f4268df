"""CPU: the C-ABI library builds, loads and exports every symbol that
include/ctrhip.h declares; the product refuses to run without a HIP device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ctr_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = _declared_symbols()
    assert "ctr_embed_fwd" in names and "ctr_linear_bwd" in names
    handle = lib.load()
    for name in names:
        assert hasattr(handle, name), f"{name} declared in ctrhip.h but not exported"
        assert name in lib.SIGNATURES, f"{name} has no ctypes signature in _lib.SIGNATURES"
    assert sorted(lib.SIGNATURES) == names


def test_code_object_targets_gfx950_only(lib):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o",
                          f"--input={lib.LIB_PATH}"], capture_output=True, text=True)
    if out.returncode == 0 and out.stdout.strip():
        targets = [t for t in out.stdout.split() if "amdgcn" in t]
        assert targets and all("gfx950" in t for t in targets), out.stdout
    assert lib.load().ctr_target_arch() == b"gfx950"


def test_field_struct_matches_header_size(lib):
    # 6 int32 + 2 int64 + 6 pointers + 1 int64 = 96 bytes, as ctr_field_t
    assert ctypes.sizeof(lib.Field) == 96
    # 3 pointers + int64 + 2 pointers + 4 int32 = 64 bytes, as ctr_mlp_layer_t
    assert ctypes.sizeof(lib.MlpLayer) == 64
    # pointer + int64 + 3 pointers + int64 + 2 int32 = 56 bytes, as ctr_mlp_head_t
    assert ctypes.sizeof(lib.MlpHead) == 56
    # 11 pointers / int64 + 2 int32 = 96 bytes, as ctr_mlp_head_grad_t
    assert ctypes.sizeof(lib.MlpHeadGrad) == 96
    # pointer + pointer + int64 + 4 pointers + 4 int32 = 72 bytes, as ctr_head_fold_t
    assert ctypes.sizeof(lib.HeadFold) == 72
    # 9 pointers / int64 + 4 int32 = 88 bytes, as ctr_head_fold_grad_t
    assert ctypes.sizeof(lib.HeadFoldGrad) == 88
    # ctr_ncf_proj_t / ctr_ncf_proj_grad_t: the library reports its own sizeof through an empty-batch refusal-free
    # probe is not possible without a GPU; the sizes below are the header's (11 x 8 + 8 + 4 x 64 + 3 x 8 + 8 + 2 x 8 +
    # 8 + 2 x 8 + 8 + 4 x 8 + 8 = 480; 2 x 8 + 4 x 64 + 13 x 8 = 376) and are asserted against a compiled probe
    assert ctypes.sizeof(lib.NcfProj) == _c_sizeof("ctr_ncf_proj_t")
    assert ctypes.sizeof(lib.NcfProjGrad) == _c_sizeof("ctr_ncf_proj_grad_t")


def _c_sizeof(type_name):
    """sizeof(type) as a C compiler sees include/ctrhip.h"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write(f'#include <stdio.h>\n#include "ctrhip.h"\nint main(void) {{ printf("%zu", sizeof({type_name})); return 0; }}\n')
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        return int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)


def test_strerror(lib):
    h = lib.load()
    assert h.ctr_strerror(0) == b"ok"
    assert b"invalid" in h.ctr_strerror(-1)


def test_argument_validation_without_gpu(lib):
    # host-side checks run before any launch: null pointers / bad sizes are refused
    h = lib.load()
    assert h.ctr_embed_fwd(None, 0, None, 0, 4, None, 0, None, None) == -1
    assert h.ctr_linear_fwd(None, 0, None, 0, None, None, 0, None, 0, 4, 4, 4, 0, None) == -1
    assert h.ctr_mf_fwd(None, 0, None, 0, 0, None, None, 4, None, None, None) == -1
    # an empty batch is a no-op, whatever the pointers are
    assert h.ctr_mf_fwd(None, 0, None, 0, 0, None, None, 0, None, None, None) == 0


def test_no_cpu_fallback(lib):
    from deeplearningrecommendationsystem_amd.model import MatrixFactorization, NeuralCF
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    with pytest.raises(CtrHipError):
        MatrixFactorization(5, 6, 4)(torch.tensor([1]), torch.tensor([2]))
    with pytest.raises(CtrHipError):
        NeuralCF(5, 6, 4, [8, 4])(torch.tensor([1]), torch.tensor([2]))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "deeplearningrecommendationsystem_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(base, f)).read()
                assert "oracle" not in src.replace("no oracle", ""), f"{f} mentions the oracle"


def test_every_environment_switch_is_documented():
    """every variable the kernels or the package read is a row of dev/README.md's switch table, so tunables and
    ablations cannot come back into the product build unnoticed"""
    pkg = os.path.join(ROOT, "deeplearningrecommendationsystem_amd")
    read = {}
    csrc = os.path.join(pkg, "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".inc")):
            for name in re.findall(r'\bgetenv\(\s*"([A-Za-z0-9_]+)"\s*\)', open(os.path.join(csrc, f)).read()):
                read.setdefault(name, f)
    py_read = re.compile(r"""os\.(?:environ\.get\(|environ\[|getenv\()\s*["']([A-Za-z0-9_]+)["']""")
    for base, _, files in os.walk(pkg):
        for f in sorted(files):
            if f.endswith(".py"):
                for name in py_read.findall(open(os.path.join(base, f)).read()):
                    read.setdefault(name, os.path.relpath(os.path.join(base, f), ROOT))
    assert {"CTR_MLP_16", "CTR_EMBED_HOT", "CTR_NCF_PROJ", "CTRHIP_LIB"} <= set(read), sorted(read)
    doc = open(os.path.join(ROOT, "dev", "README.md")).read()
    table = doc[doc.index("## A/B switches"):]
    table = table[:table.index("\n## ")] if "\n## " in table else table
    documented = set()
    for line in table.splitlines():
        if line.startswith("| `"):
            documented.update(re.findall(r"`([A-Za-z0-9_]+)`", line.split("|")[1]))
    missing = {name: where for name, where in read.items() if name not in documented}
    assert not missing, f"environment switches missing from dev/README.md's switch table: {missing}"


def _parse_header_prototypes():
    """{name: (ret, [arg ctypes])} derived from the declarations in include/ctrhip.h"""
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"(const\s+char\s*\*|int)\s+(ctr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        kinds = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "ctr_field_t" in a:
                    kinds.append("field*")
                elif "ctr_ncf_proj_grad_t" in a:
                    kinds.append("ncfprojgrad*")
                elif "ctr_ncf_proj_t" in a:
                    kinds.append("ncfproj*")
                elif "ctr_mlp_layer_t" in a:
                    kinds.append("mlp*")
                elif "ctr_mlp_head_grad_t" in a:
                    kinds.append("headgrad*")
                elif "ctr_mlp_head_t" in a:
                    kinds.append("head*")
                elif "ctr_head_fold_grad_t" in a:
                    kinds.append("foldgrad*")
                elif "ctr_head_fold_t" in a:
                    kinds.append("fold*")
                elif "ctr_adam_tensor_t" in a:
                    kinds.append("adam*")
                elif "ctr_rows_mark_t" in a:
                    kinds.append("mark*")
                elif "ctr_rows_table_t" in a:
                    kinds.append("rows*")
                elif a.startswith("float "):
                    kinds.append("f32")
                elif a.startswith("double "):
                    kinds.append("f64")
                elif "int32_t*" in a.replace(" *", "*") and "const" in a:
                    kinds.append("i32*")
                elif "*" in a:
                    kinds.append("ptr")
                elif a.startswith("int64_t"):
                    kinds.append("i64")
                elif a.startswith("uint64_t"):
                    kinds.append("u64")
                elif a.startswith("int ") or a.startswith("int32_t "):
                    kinds.append("int")
                else:
                    raise AssertionError(f"unparsed parameter {a!r} of {name}")
        protos[name] = ("str" if "char" in ret else "int", kinds)
    return protos


def test_ctypes_signatures_match_header_prototypes(lib):
    protos = _parse_header_prototypes()
    assert set(protos) == set(lib.SIGNATURES)
    to_kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int: "int", ctypes.c_char_p: "str"}
    for name, (ret, kinds) in protos.items():
        res, args = lib.SIGNATURES[name]
        assert to_kind[res] == ret, name
        got = []
        for a in args:
            if a in to_kind:
                got.append(to_kind[a])
            elif a is ctypes.POINTER(lib.Field):
                got.append("field*")
            elif a is ctypes.POINTER(lib.MlpLayer):
                got.append("mlp*")
            elif a is ctypes.POINTER(lib.NcfProj):
                got.append("ncfproj*")
            elif a is ctypes.POINTER(lib.NcfProjGrad):
                got.append("ncfprojgrad*")
            elif a is ctypes.POINTER(lib.MlpHead):
                got.append("head*")
            elif a is ctypes.POINTER(lib.MlpHeadGrad):
                got.append("headgrad*")
            elif a is ctypes.POINTER(lib.HeadFold):
                got.append("fold*")
            elif a is ctypes.POINTER(lib.HeadFoldGrad):
                got.append("foldgrad*")
            elif a is ctypes.POINTER(lib.AdamTensor):
                got.append("adam*")
            elif a is ctypes.POINTER(lib.RowsMark):
                got.append("mark*")
            elif a is ctypes.POINTER(lib.RowsTable):
                got.append("rows*")
            elif a is ctypes.c_float:
                got.append("f32")
            elif a is ctypes.c_double:
                got.append("f64")
            elif a is ctypes.c_uint64:
                got.append("u64")
            elif a is ctypes.POINTER(ctypes.c_int32):
                got.append("i32*")
            elif a in (ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)):
                got.append("ptr")  # host arrays of device pointers / of sizes (ctr_fields_*)
            else:
                raise AssertionError(f"{name}: unexpected ctypes arg {a}")
        # a device `int32_t* err_flag` is passed as a raw pointer; only host int arrays are typed
        norm = ["ptr" if k == "i32*" and g == "ptr" else k for k, g in zip(kinds, got)]
        assert got == norm, f"{name}: header {kinds} vs ctypes {got}"


def test_python_mirrors_of_header_limits_match(lib):
    """the admission checks on the Python side (ops.NcfProj.supported(), ops.topk_rows, ...) read these mirrors: a
    limit changed in the header alone would send admitted shapes to a library that refuses them"""
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    defines = _header_defines(text)
    for name in ("CTR_MAX_FIELDS", "CTR_NCF_PROJ_MAX_ROWS", "CTR_NCF_PROJ_COUNT_STRIDE", "CTR_ROWS1_MAX_ROWS"):
        assert getattr(lib, name) == defines[name], name
    assert ops.TOPK_MAX_K == defines["CTR_TOPK_MAX_K"]
    # every mirror, not a chosen few: an int under a CTR_ name in _lib is a define of the header, and equal to it
    mirrors = {name: value for name, value in vars(lib).items()
               if name.startswith("CTR_") and isinstance(value, int) and not isinstance(value, bool)}
    assert len(mirrors) >= 34 and {"CTR_TOPK_MAX_K", "CTR_RANK_MAX_ROWS", "CTR_ELIMIT"} <= set(mirrors)
    for name, value in mirrors.items():
        assert name in defines, f"_lib.{name} mirrors nothing: include/ctrhip.h has no such #define"
        assert value == defines[name], f"_lib.{name} = {value}, the header says {defines[name]}"


def _header_defines(text):
    """{name: int} of every object-like ``#define CTR_*`` of the header whose value is an integer: decimal, hex with a
    ``u`` suffix, ``(1ll << n)`` or a parenthesised negative; a trailing comment may follow"""
    forms = ((r"(\d+)", int), (r"(0[xX][0-9a-fA-F]+)u", lambda v: int(v, 16)),
             (r"\(1ll << (\d+)\)", lambda v: 1 << int(v)), (r"\((-\d+)\)", int))
    defines = {}
    for name, value in re.findall(r"^#define[ \t]+(CTR_[A-Z0-9_]+)[ \t]+(.+)$", text, flags=re.M):
        value = re.sub(r"/\*.*|//.*", "", value).strip()
        for pattern, convert in forms:
            m = re.fullmatch(pattern, value)
            if m:
                defines[name] = convert(m.group(1))
    return defines


def test_header_define_parser_reads_every_form():
    got = _header_defines("#define CTR_A 12   /* twelve */\n#define CTR_B 0xffffffffu\n#define CTR_C (1ll << 24)\n"
                          "#define CTR_D (-4)  /* d */\n#define CTR_E  7 // e\n#define CTR_F(x) (2 * (x))\n"
                          "#define CTR_G 1.5f\n#define OTHER 3\n")
    assert got == dict(CTR_A=12, CTR_B=0xFFFFFFFF, CTR_C=1 << 24, CTR_D=-4, CTR_E=7)
