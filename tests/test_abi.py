"""The C-ABI library loads and exports every symbol include/adafortitran_amd.h declares
(no compute calls: this runs without a GPU)."""
import ctypes
import os
import re

import pytest

from adafortitran_amd import _abi, _lib
from helpers import DEFAULT_SPEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    """The header without comments."""
    text = open(os.path.join(ROOT, "include", "adafortitran_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _header_symbols():
    return sorted(set(re.findall(r"\b(aft_[a-z0-9_]+)\s*\(", _header_text())))


def test_binding_lists_every_header_symbol():
    assert _header_symbols() == sorted(_abi.EXPORTED_SYMBOLS)


# ---- the binding against the header, declaration by declaration (no library, no GPU) ----
# What ctypes can get wrong without raising is the KIND of a value: its width, integer or floating point, by value or by address.
_C_KINDS = {"int": "i32", "int32_t": "i32", "size_t": "u64", "uint64_t": "u64", "unsigned long long": "u64", "long long": "i64",
            "float": "f32", "double": "f64"}
_CTYPES_KINDS = {ctypes.c_int: "i32", ctypes.c_size_t: "u64", ctypes.c_uint64: "u64", ctypes.c_ulonglong: "u64",
                 ctypes.c_longlong: "i64", ctypes.c_float: "f32", ctypes.c_double: "f64"}
_C_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
_MIRRORS = {"aft_config": _abi.AftConfig, "aft_layer_weights": _abi.AftLayerWeights, "aft_weights": _abi.AftWeights,
            "aft_chansim": _abi.AftChanSim, "aft_lmmse": _abi.AftLmmse, "aft_link": _abi.AftLink, "aft_layer_grads": _abi.AftLayerGrads,
            "aft_step_control": _abi.AftStepControl}
_STRUCTS_PASSED_AS_VOID_P = {"aft_step_control"}        # optim.py keeps the control block in a tensor and passes its address


def _header_constants():
    """{name: value} of every ``#define AFT_NAME <integer>`` and every enumerator."""
    text = _header_text()
    define = r"^[ \t]*#[ \t]*define[ \t]+(AFT_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$"
    found = {n: int(v, 0) for n, v in re.findall(define, text, flags=re.M)}
    for body in re.findall(r"\benum\b[^{;]*\{(.*?)\}", text, flags=re.S):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, given = (part.strip() for part in item.partition("="))
            value = int(given, 0) if given else value + 1
            found[name] = value
    return found


def _c_declarations(statement, what):
    """'const float *enh_w[4], *enh_b[4]' -> [(name, kind, array extents, struct named or None), ...] for one C declaration
    (a struct's field list or one parameter).  A pointer's extents are those of the array OF pointers; a type passed by value that
    this test does not know fails it."""
    defines = _header_constants()
    first, *more = (d.strip() for d in statement.split(","))
    m = re.fullmatch(r"(?P<base>[\w ]+?)\s*(?P<decl>(?:\*\s*(?:const\s+)?)?\w+\s*(?:\[\w*\]\s*)*)", first)
    assert m, f"{what}: cannot read {statement!r}"
    base = " ".join(w for w in m["base"].split() if w != "const")
    out = []
    for decl in (m["decl"], *more):
        d = re.fullmatch(r"(?P<star>\*?)\s*(?:const\s+)?(?P<name>\w+)\s*(?P<dims>(?:\[\w*\]\s*)*)", decl)
        assert d, f"{what}: cannot read {decl!r} in {statement!r}"
        dims = re.findall(r"\[(\w*)\]", d["dims"])
        struct = base if base in _MIRRORS else None
        assert d["star"] or struct or base in _C_KINDS, f"{what}: unknown C type {base!r} in {statement!r}"
        kind = "pointer" if d["star"] else "struct" if struct else _C_KINDS[base]
        out.append((d["name"], kind, [int(x) if x.isdigit() else defines[x] for x in dims], struct))
    return out


def _ctypes_declaration(t):
    """(kind, array extents outermost first, struct class a POINTER names or None) of one ctypes type."""
    extents = []
    while issubclass(t, ctypes.Array):
        extents.append(t._length_)
        t = t._type_
    if issubclass(t, ctypes._Pointer):
        return "pointer", extents, t._type_ if issubclass(t._type_, ctypes.Structure) else None
    if t in (ctypes.c_void_p, ctypes.c_char_p):
        return "pointer", extents, None
    assert t in _CTYPES_KINDS, f"{t} is not a type this test knows"
    return _CTYPES_KINDS[t], extents, None


def _header_prototypes():
    """[(name, return type, [parameter text, ...]), ...] in the header's order."""
    text = re.sub(r"^[ \t]*#.*$", "", _header_text(), flags=re.M)
    protos = []
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(aft_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        protos.append((name, " ".join(ret.split()), [] if params == ["void"] else params))
    return protos


def test_signatures_match_the_header_prototypes():
    """Every line of _abi.SIGNATURES against its prototype: the number of arguments, the kind of each (pointer / i32 / u64 / i64 / f32
    / f64 -- two arguments of one width but different kinds swapped pass ctypes and hand a kernel a wild address), the return type
    (a size_t query typed c_int is cut to 32 bits), and the mirror class behind every pointer to one of the ABI's structs."""
    protos = _header_prototypes()
    assert len(protos) == len(_abi.SIGNATURES) and len(protos) >= 56       # a pattern that stopped matching cannot pass
    assert [name for name, _, _ in protos] == list(_abi.SIGNATURES)         # exactly once each, in the header's order
    for name, ret, params in protos:
        restype, argtypes = _abi.SIGNATURES[name]
        assert ret in _C_RETURNS, f"{name}: unknown return type {ret!r}"
        assert restype is _C_RETURNS[ret], f"{name}: returns {ret}, bound as {restype}"
        assert len(params) == len(argtypes), f"{name}: {len(params)} parameters, {len(argtypes)} argtypes"
        for i, (param, argtype) in enumerate(zip(params, argtypes)):
            (_, kind, dims, struct), = _c_declarations(param, name)
            kind = "pointer" if dims else kind                              # an array parameter is a pointer
            assert kind != "struct", f"{name}: {param!r} passes a struct by value"
            bound, extents, target = _ctypes_declaration(argtype)
            assert not extents and bound == kind, f"{name} argument {i} ({param!r}): {kind} in the header, {argtype} in the binding"
            want = None if struct in _STRUCTS_PASSED_AS_VOID_P else _MIRRORS.get(struct)
            assert target is want, f"{name} argument {i} ({param!r}): bound as a pointer to {target}, not {want}"


def test_struct_mirrors_match_the_header_field_by_field():
    """Every typedef'd struct of the header against its ctypes mirror: the same field names in the same order, each of the same kind
    and array extent (resolved through the header's own #defines), a pointer to another struct typed as that struct's mirror."""
    structs = re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", _header_text(), flags=re.S)
    assert sorted(name for _, name in structs) == sorted(_MIRRORS) and len(structs) == 8
    for body, name in structs:
        fields = [f for stmt in body.split(";") if stmt.strip() for f in _c_declarations(" ".join(stmt.split()), name)]
        mirror = _MIRRORS[name]._fields_
        assert [f[0] for f in fields] == [m[0] for m in mirror], name
        for (fname, kind, dims, struct), (_, ctype) in zip(fields, mirror):
            assert kind != "struct", f"{name}.{fname}: a struct by value"
            bound, extents, target = _ctypes_declaration(ctype)
            assert (bound, extents) == (kind, dims), f"{name}.{fname}: {kind}{dims} in the header, {bound}{extents} in the mirror"
            assert target is _MIRRORS.get(struct), f"{name}.{fname}: mirrored as a pointer to {target}"


def test_constants_match_the_header():
    """Every integer #define / enumerator of the header that _abi mirrors carries the header's value there, and _abi mirrors no
    AFT_* constant the header does not have."""
    header = _header_constants()
    compared = {n: v for n, v in header.items() if hasattr(_abi, n)}
    assert compared and "AFT_ABI_VERSION" in compared
    assert {n for n in vars(_abi) if n.startswith("AFT_")} == set(compared)
    for n, v in compared.items():
        assert getattr(_abi, n) == v, f"{n}: {v} in the header, {getattr(_abi, n)} in _abi"


def test_library_exports_all_symbols():
    import torch  # noqa: F401  (binds libamdhip64.so.7 the way the product does)
    assert os.path.exists(_lib.lib_path()), "build with python -m adafortitran_amd.build"
    lib = ctypes.CDLL(_lib.lib_path())
    for name in _header_symbols():
        assert hasattr(lib, name), name


def test_loader_checks_version_and_host_only_calls():
    lib = _lib.load()
    assert lib.aft_version() == _abi.AFT_ABI_VERSION
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=(7, 42, 560))
    nbytes = lib.aft_workspace_bytes(ctypes.byref(cfg), 128)
    # conv_enhanced + tokens6 + x + attn + q + k + vt at B=128 (DESIGN.md data layout)
    planes, tokens, tokpad, d = 256, 280, 288, 128
    # conv_enhanced + tokens6 + x + attn + q + k + vt + fragment-packed encoder weights (6 layers x 8 d^2)
    # + linear_2 output of the last chain launch (rows x 8)
    # (the attention tiles are sized like a whole q / k / v^T block, planes x tokpad rows: the fused layer sequence uses the
    # region as its second K buffer)
    expect = 4 * (planes * 1680 + 128 * tokens * 6 + planes * tokens * d + planes * tokpad * d + 3 * planes * 4 * tokpad * 32
                  + 6 * 8 * d * d + planes * tokens * 8 + 2 * (22 * 64 * 4 + 160))   # + both conv stacks' 16x16x4 operand fragments and helper tables
    # ABI 6: the forward may run as up to AFT_MAX_LANES = 4 shares of the batch, each with its own packed weights and fragment tables
    # (aft_workspace_lanes); the size covers whichever split the call picks
    expect += 4 * 3 * (6 * 8 * d * d + 2 * (22 * 64 * 4 + 160))
    assert expect <= nbytes <= expect + 40 * 256
    for d, heads in ((84, 4), (520, 8), (4, 1)):        # not a multiple of 8 / above 512 / below 8
        bad = _abi.make_config(**dict(DEFAULT_SPEC, model_dim=d, num_head=heads))
        assert lib.aft_workspace_bytes(ctypes.byref(bad), 8) == 0 and lib.aft_engine_of(ctypes.byref(bad)) < 0
        assert b"model_dim" in lib.aft_last_error()
    # ABI 7: two engines behind one call.  The packed engine's shapes (model_dim a multiple of 32 up to 256, head dims that are multiples
    # of 8 up to 64 except 56); everything else nn.TransformerEncoderLayer builds up to model_dim 512 / head dim 128 runs the general one;
    # a num_head that does not divide model_dim (torch refuses it too) and heads above 128 features are refused with the reason
    P, G = _abi.AFT_ENGINE_PACKED, _abi.AFT_ENGINE_GENERAL
    for d, heads, engine in ((128, 4, P), (128, 16, P), (96, 4, P), (192, 4, P), (160, 4, P), (256, 8, P), (224, 4, G), (96, 8, G), (128, 1, G),
                             (160, 8, G), (512, 8, G), (512, 4, G), (384, 4, G), (80, 5, G), (200, 8, G), (120, 8, G), (128, 3, -1), (512, 2, -1)):
        c = _abi.make_config(**dict(DEFAULT_SPEC, model_dim=d, num_head=heads))
        assert lib.aft_engine_of(ctypes.byref(c)) == engine, (d, heads)
        assert (lib.aft_workspace_bytes(ctypes.byref(c), 8) > 0) == (engine >= 0), (d, heads)
        assert engine >= 0 or b"head dim" in lib.aft_last_error()
    # patches: up to 16 elements packed, up to 32 general, more refused; any layer count
    for patch, engine in (((3, 2), P), ((4, 2), P), ((8, 2), P), ((12, 2), G), ((8, 7), -1)):
        c = _abi.make_config(**dict(DEFAULT_SPEC, ofdm=(96, 14), pilot=(12, 2), patch=patch))
        assert lib.aft_engine_of(ctypes.byref(c)) == engine, patch
    for layers in (1, 33, 100):
        c = _abi.make_config(**dict(DEFAULT_SPEC, num_layers=layers))
        assert lib.aft_engine_of(ctypes.byref(c)) == P and lib.aft_workspace_bytes(ctypes.byref(c), 4) > 0


def test_switches_are_read_once_and_change_through_the_abi_only(switches):
    """no getenv() on a call path.  The library snapshots the AFT_* environment when it is loaded; afterwards a switch
    changes through aft_set_switch only -- os.environ is not consulted again."""
    lib = _lib.load()
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=(7, 42, 560))

    def lanes(batch):
        n, frames, offs = ctypes.c_int(), (ctypes.c_int * 4)(), (ctypes.c_size_t * 4)()
        assert lib.aft_workspace_lanes(ctypes.byref(cfg), batch, ctypes.byref(n), frames, offs) == _abi.AFT_OK
        return n.value

    switches.unset("AFT_LANES")
    base = lanes(64)
    os.environ["AFT_LANES"] = "3"
    try:
        assert lanes(64) == base and _lib.get_switch("AFT_LANES") is None       # the environment no longer matters
    finally:
        del os.environ["AFT_LANES"]
    switches.set("AFT_LANES", 3)
    assert lanes(64) == 3 and _lib.get_switch("AFT_LANES") == "3"
    with _lib.switch("AFT_LANES", 1):
        assert lanes(64) == 1
    assert lanes(64) == 3
    with pytest.raises(ValueError):
        _lib.set_switch("PATH", "x")              # only AFT_* names


def test_unknown_switch_names_are_refused():
    """A misspelled switch must not pass silently (a test that sets one would compare the product path with itself):
    aft_set_switch refuses a name csrc/switches.h does not declare, aft_get_switch returns -1 for it."""
    for name in ("AFT_LANE", "AFT_TRAIN_UNFUSED_FORWARD", "AFT_ATTN_HD16_MFMA32", "AFT_CONV_MFMA32", "AFT_BATCH", "PATH"):
        with pytest.raises(ValueError, match=name):
            _lib.set_switch(name, "1")
        with pytest.raises(ValueError, match=name):
            _lib.get_switch(name)
        with pytest.raises(ValueError):
            with _lib.switch(name, 1):
                pass
    bogus = b"AFT_NOT_A_SWITCH"
    assert _lib.load().aft_get_switch(bogus, None, 0) == -1


def test_every_switch_the_repository_names_is_declared(switches):
    """Every name bench.py, tests/ and tools/ hand to set_switch / get_switch, _lib.switch(...), the `switches` fixture or
    aft_set_switch is a declared switch (the library accepts it and reads it back)."""
    call = re.compile(r"(?:set_switch|get_switch|_lib\.switch|switches\.set|switches\.unset)\(\s*b?[\"'](AFT_[A-Z0-9_]+)[\"']")
    files = [os.path.join(ROOT, "bench.py")]
    for top in ("tests", "tools"):
        for base, _, names in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(base, n) for n in names if n.endswith((".py", ".sh"))]
    used = set()
    for path in files:
        used.update(call.findall(open(path, errors="replace").read()))
    assert {"AFT_LANES", "AFT_PROLOGUE_NO_UP", "AFT_CONV_NSPLIT", "AFT_ALLOW_COMPOSITE", "AFT_STAMPS"} <= used, used
    for name in sorted(used):
        switches.set(name, "7")
        assert _lib.get_switch(name) == "7", name


def test_lanes_split_the_batch_into_contiguous_shares_inside_the_workspace(switches):
    """aft_workspace_lanes: the shares a forward of `batch` frames runs as (include/adafortitran_amd.h "Lanes"): contiguous,
    non-empty, slices laid end to end and inside aft_workspace_bytes -- which must not depend on AFT_LANES (read per call)."""
    lib = _lib.load()
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=(7, 42, 560))

    def plan(batch):
        lanes, frames, offs = ctypes.c_int(), (ctypes.c_int * 4)(), (ctypes.c_size_t * 4)()
        assert lib.aft_workspace_lanes(ctypes.byref(cfg), batch, ctypes.byref(lanes), frames, offs) == _abi.AFT_OK
        return lanes.value, list(frames)[:lanes.value], list(offs)[:lanes.value]

    switches.unset("AFT_LANES")
    sizes = {b: lib.aft_workspace_bytes(ctypes.byref(cfg), b) for b in (1, 2, 7, 64, 128)}
    # two lanes between one row tile per CU and ~15, unless one lane's launches are nearly whole rounds of the persistent grids
    # (127 / 128 frames of the default model); 8 frames: 140 row tiles, less than one per CU.  The rule is written in CUs: the exact
    # decisions below hold for the MI355X's 256 (also the library's answer when no device is visible); on any other part only the
    # invariants are asserted
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    decisions = [plan(b)[0] for b in (1, 8, 16, 64, 96, 120, 127, 128, 129, 192, 224, 256, 512)]
    assert decisions[0] == 1 and set(decisions) <= {1, 2}
    if cus == 256:
        assert decisions == [1, 1, 2, 2, 2, 2, 1, 1, 2, 2, 2, 1, 1]
    for want in (1, 2, 3, 4):
        switches.set("AFT_LANES", str(want))
        for batch, total in sizes.items():
            assert lib.aft_workspace_bytes(ctypes.byref(cfg), batch) == total
            n, frames, offs = plan(batch)
            assert n == min(want, batch) and sum(frames) == batch and min(frames) > 0 and max(frames) - min(frames) <= 1
            assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and offs == sorted(offs)
            # the last slice ends inside the workspace: its own size is at most aft_workspace_bytes(its frames), which allows for
            # three more copies of the packed weights and fragment tables than one unsplit forward needs
            slack = 4 * 3 * (6 * 8 * 128 * 128 + 2 * (22 * 64 * 4 + 160)) + 40 * 256
            assert offs[-1] + lib.aft_workspace_bytes(ctypes.byref(cfg), frames[-1]) - slack <= total
    lanes = ctypes.c_int()
    assert lib.aft_workspace_lanes(ctypes.byref(cfg), 0, ctypes.byref(lanes), None, None) == _abi.AFT_ERR_ARG


def test_workspace_regions_are_inside_the_workspace():
    lib = _lib.load()
    cfg = _abi.make_config(**DEFAULT_SPEC, adaptive_hidden=(7, 42, 560))
    total = lib.aft_workspace_bytes(ctypes.byref(cfg), 8)
    spans = {}
    for name, rid in _abi.REGION_IDS.items():
        off, size = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.aft_workspace_region(ctypes.byref(cfg), 8, rid, ctypes.byref(off), ctypes.byref(size)) == _abi.AFT_OK
        assert off.value % 256 == 0 and off.value + size.value <= total
        spans[name] = (off.value, size.value)
    assert spans["conv_enhanced"] == (0, 4 * 16 * 120 * 14)
    assert spans["tokens6"][1] == 4 * 8 * 280 * 6 and spans["enc_out"][1] == 4 * 16 * 280 * 8
    off, size = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.aft_workspace_region(ctypes.byref(cfg), 8, 99, ctypes.byref(off), ctypes.byref(size)) == _abi.AFT_ERR_ARG
    assert lib.aft_workspace_region(ctypes.byref(cfg), 0, 0, ctypes.byref(off), ctypes.byref(size)) == _abi.AFT_ERR_ARG


def test_struct_sizes_match_header():
    assert ctypes.sizeof(_abi.AftConfig) == 16 * 4
    assert ctypes.sizeof(_abi.AftLayerWeights) == 12 * 8
    n_ptrs = 2 + 8 + 8 + 18 + 2 + 1 + 2
    assert ctypes.sizeof(_abi.AftWeights) == (n_ptrs + 1) * 8          # + the host pointer to the layer table (ABI 7: any layer count)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.AftError, match="no CPU or PyTorch fallback"):
        _lib.load()


def test_max_batch_is_the_32_bit_offset_limit_of_the_largest_region():
    """aft_max_batch (host-only): the q / k / v^T blocks and the attention tiles are planes x tokpad x d floats and must
    stay under 2 GiB; one frame more is refused by aft_forward_f32 before anything is launched."""
    lib = _lib.load()
    for spec, hid, tokpad in ((DEFAULT_SPEC, (7, 42, 560), 288),
                              (dict(ofdm=(240, 28), pilot=(24, 4), patch=(3, 2), num_layers=12, model_dim=256, num_head=8),
                               (7, 42, 2240), 1120)):
        cfg = _abi.make_config(**spec, adaptive_hidden=hid)
        mb = lib.aft_max_batch(ctypes.byref(cfg))
        per_frame = 2 * tokpad * spec["model_dim"] * 4
        assert mb == (2 ** 31 - 1) // per_frame
        assert lib.aft_workspace_bytes(ctypes.byref(cfg), mb) > 0
        w = _abi.AftWeights()
        table = (_abi.AftLayerWeights * spec["num_layers"])()
        w.layers = ctypes.cast(table, ctypes.POINTER(_abi.AftLayerWeights))
        one = ctypes.c_float(0.0)
        ptr = ctypes.addressof(one)                       # non-NULL dummies: the call must fail before touching them
        rc = lib.aft_forward_f32(ctypes.byref(cfg), ctypes.byref(w), ptr, ptr, ptr, ptr, ptr, ptr, 1 << 40, mb + 1, None)
        assert rc == _abi.AFT_ERR_ARG and b"aft_max_batch" in lib.aft_last_error()
    bad = _abi.make_config(**dict(DEFAULT_SPEC, model_dim=640, num_head=10), adaptive_hidden=None)
    assert lib.aft_max_batch(ctypes.byref(bad)) == 0 and lib.aft_packed_weights_bytes(ctypes.byref(bad)) == 0
    wide = _abi.make_config(**dict(DEFAULT_SPEC, model_dim=512, num_head=4), adaptive_hidden=None)      # general engine: its largest tensor
    assert lib.aft_max_batch(ctypes.byref(wide)) == (2 ** 31 - 1) // (2 * 280 * 3 * 512 * 4)             # is q | k | v, rows x 3 d floats
    assert lib.aft_packed_weights_bytes(ctypes.byref(wide)) > 0


def test_hot_kernels_have_no_register_spills():
    """hipcc's own resource report for the two hot kernels that have tripped before (an innocent-looking extra instantiation of the
    attention body's steady-state step spilled 150 VGPRs and cost 33 % of the kernel's speed, round 4): the tuned head-dim-32
    attention kernel, both column-streaming conv kernels and the row-local training kernels must not spill a single vector
    register; the head-dim-64 attention instantiation (two blocks of q / k / v^T, two accumulators, 256 VGPRs) may spill at most a couple."""
    import re
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adafortitran_amd", "csrc")
    report = {}
    for src in ("k_attn.hip", "k_conv_stream.hip", "k_conv_rows.hip", "k_chain_bwd.hip"):
        res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", "/dev/null",
                              "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        name = None
        for line in res.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            m = re.search(r"VGPRs Spill: (\d+)", line)
            if m and name:
                report[name] = int(m.group(1))
    spills = {k: v for k, v in report.items() if "attn_kernelILi32E" in k or "attn16_kernel" in k or "conv_stream16_kernel" in k}
    # attention HD 32 (generic, 280 tokens, 1120 tokens), conv stream head / tail / training (conv_stream16_kernel x 1 / 2 / 4 column
    # ranges), attn16_kernel<0 | 280, 16 | 8>: head dims 16 / 8 on 16x16x4 MFMAs
    assert len(spills) == 16 and all(v == 0 for v in spills.values()), report
    # the 32x32x2 streaming conv kernels are retired: the default grid and tall planes run the 16x16x4 ones only
    assert not any("conv_stream_kernelI" in k or "conv_rows_kernelI" in k for k in report), report
    # the 32x32x2 forms of head dims 16 and 8 are retired: those heads run attn16_kernel only
    assert not any("attn_kernelILi16E" in k or "attn_kernelILi8E" in k for k in report), report
    assert all(v <= 4 for k, v in report.items() if "attn_kernelILi64E" in k), report
    # the row-local training kernels (forward chain with / without the in-projection tail, backward chain; gelu and relu) sit at the
    # 168 registers three waves per SIMD allow: a scratch reload is a VMEM load whose wait drains vmcnt
    chain = {k: v for k, v in report.items() if "chain_fwd_train_kernel" in k or "chain_bwd_kernel" in k}
    assert len(chain) == 8 and all(v == 0 for v in chain.values()), report      # forward: act x tail; backward: act x partial-last-tile
    rows = {k: v for k, v in report.items() if "conv_rows16_kernel" in k}    # head / tail of the row-streaming conv kernel (246 VGPRs)
    assert len(rows) == 2 and all(v == 0 for v in rows.values()), report
