"""CPU-only: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/matinvent_hip.h (the boundary) and include/matinvent_hip_debug.h (experiment knobs) declare -- no compute calls without a GPU."""
import ctypes
import os

from matinvent_amd import _lib
from matinvent_amd.build import build
from tests.header_util import INCLUDE, ROOT, declared_symbols


def test_library_builds_and_exports_every_declared_symbol():
    path = build(verbose=False)
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    names = declared_symbols()
    debug = declared_symbols("matinvent_hip_debug.h")
    assert len(names) >= 20
    # the product header carries the boundary only; every experiment knob lives in the debug header, and only there
    assert not [n for n in names if n.startswith("mi_debug_")] and all(n.startswith("mi_debug_") for n in debug)
    assert len(names) <= 65
    for n in names + debug:
        assert hasattr(lib, n), f"{n} declared in include/ but not exported"
    # the ctypes table binds exactly the declared set (both headers)
    assert sorted(_lib.SIGNATURES) == sorted(names + debug)


def test_every_public_header_is_bound_by_exactly_one_table_and_loaded():
    """Every symbol of every include/*.h is a key of exactly one _lib table, and load() attached that table's restype / argtypes: a table
    that is defined but left out of load()'s loop would leave its entries with ctypes' defaults."""
    tables = (_lib.SIGNATURES,) + _lib.EXTENSION_SIGNATURES
    assert any(t is _lib.TRAJ_SIGNATURES for t in tables) and any(t is _lib.PG_SIGNATURES for t in tables)
    assert any(t is _lib.PG_KL_SIGNATURES for t in tables)
    headers = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
    assert len(headers) >= 5
    build(verbose=False)
    lib = _lib.load()
    declared = []
    for h in headers:
        names = declared_symbols(h)
        assert names, h
        declared += names
        for n in names:
            owners = [t for t in tables if n in t]
            assert len(owners) == 1, f"{n} ({h}) is bound by {len(owners)} tables"
            res, args = owners[0][n]
            fn = getattr(lib, n)
            assert fn.restype == res and fn.argtypes == args, f"{n} ({h}): load() did not attach its signature"
    assert len(declared) == len(set(declared))                            # no symbol declared by two headers
    assert sorted(declared) == sorted(n for t in tables for n in t)       # and no table entry without a declaration


def test_host_only_entry_points():
    lib = _lib.load()
    assert lib.mi_version() == 1
    h = ctypes.c_void_p()
    bad = _lib.NetConfig(100, 2, 8, 256, 1)
    assert lib.mi_net_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    assert b"hidden_dim" in lib.mi_last_error()
    cfg = _lib.NetConfig(512, 6, 128, 256, 1)
    _lib.check(lib.mi_net_create(ctypes.byref(cfg), ctypes.byref(h)))
    assert lib.mi_net_num_params(h) == 12346468  # SURVEY.md section 8d [PROBE]
    name, off, numel = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
    r, c = ctypes.c_int(), ctypes.c_int()
    total = 0
    for i in range(lib.mi_net_num_tensors(h)):
        _lib.check(lib.mi_net_param_info(h, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(numel), ctypes.byref(r), ctypes.byref(c)))
        assert off.value == total and off.value % 4 == 0
        total += numel.value
    assert total == 12346468
    lib.mi_net_destroy(h)


def test_retired_debug_values_are_pinned():
    """The setter values that once selected ablation-only kernel forms: the plane GEMM's DMA mode 4 and the big-tile
    segmented-sum switch are refused, the one-launch edge stage's switch selects nothing, and the first edge GEMM's form numbers 2 .. 4
    stay accepted.  Host-side state only: no GPU."""
    lib = _lib.load()
    try:
        assert lib.mi_debug_set_planes_dma(1) == 0
        assert lib.mi_debug_set_planes_dma(4) == _lib.MI_EINVAL
        assert b"mode" in lib.mi_last_error()
        assert lib.mi_debug_set_planes_dma(3) == 0   # (this setter and the next return a status, not the previous value: the refusal is what can be read)
        assert lib.mi_debug_set_planes_big_seg(1) == _lib.MI_EINVAL
        assert lib.mi_debug_set_planes_big_seg(0) == 0
        assert lib.mi_debug_set_edge_fused(1) == 0   # retired: returns 0 ...
        assert lib.mi_debug_set_edge_fused(0) == 0   # ... and the 1 before it selected nothing
        was = lib.mi_debug_set_edge1_fused(2)
        assert was == 9                               # the default
        assert lib.mi_debug_set_edge1_fused(9) == 2   # accepted: read back through the return value
        was = lib.mi_debug_set_rt_lean(2 | (5 << 2))  # (the bits above bit 1 once sized a persistent grid: ignored)
        assert lib.mi_debug_set_rt_lean(was) == 2
    finally:
        lib.mi_debug_set_planes_dma(1)
        lib.mi_debug_set_planes_big_seg(0)
        lib.mi_debug_set_edge_fused(0)
        lib.mi_debug_set_edge1_fused(9)
        lib.mi_debug_set_rt_lean(1)


def test_missing_library_fails_loudly(monkeypatch):
    import pytest
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmatinvent_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_node_chain_touch_loads_share_one_reserved_register():
    """The L2 warm-up loads of node_chain.hip are fire-and-forget inline asm; they are safe only when every one of them writes the single
    VGPR that stays reserved until the closing s_waitcnt (advisor finding, round 5).  Checked on the device assembly of THIS source."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("scan_touch_regs", os.path.join(ROOT, "scripts", "scan_touch_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report, bad = mod.scan()
    assert len(report) >= 3, report     # the three widths of node_chain_kernel
    assert not bad, bad
    assert all(n == 3 and len(regs) == 1 for _, n, regs, _ in report), report
