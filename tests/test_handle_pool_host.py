"""CPU-only checks of the batch-handle pool (include/matinvent_hip_pool.h, matinvent_amd/pool.py): the size classes, the header,
the cfg.handle_pool parser, the index-table decode on the host (scripts/pool_tables_host_check.cpp), and that creating a pool without a
GPU is an error of the library."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from matinvent_amd import _lib
from matinvent_amd.build import build
from tests.header_util import ROOT, declared_symbols

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30


def _block_bytes():
    build(verbose=False)
    from matinvent_amd.pool import block_bytes
    return block_bytes


def test_size_classes_hand_worked():
    bb = _block_bytes()
    want = {
        -5: 512, 0: 512, 1: 512, 511: 512, 512: 512, 513: 1024, 1000: 1024, 4096: 4096, 4097: 8192, 100_000: 131_072,
        MIB - 1: MIB, MIB: MIB,
        MIB + 1: MIB + 128 * KIB,                    # above 1 MiB: multiples of (1 MiB / 8) up to 2 MiB
        MIB + 128 * KIB: MIB + 128 * KIB, MIB + 128 * KIB + 1: MIB + 256 * KIB,
        2 * MIB - 1: 2 * MIB, 2 * MIB: 2 * MIB, 2 * MIB + 1: 2 * MIB + 256 * KIB,   # ... of (2 MiB / 8) up to 4 MiB
        3 * MIB: 3 * MIB, 5 * MIB: 5 * MIB, 5 * MIB + 1: 5 * MIB + 512 * KIB,
        3 * GIB + 7: 3 * GIB + 256 * MIB,            # past 2^31: 64-bit arithmetic
    }
    for req, cls in want.items():
        assert bb(req) == cls, (req, bb(req), cls)


def test_size_classes_are_monotone_cover_the_request_and_waste_at_most_an_eighth():
    bb = _block_bytes()
    reqs = sorted(set([1, 2, 511, 512, 513] + [(1 << k) + d for k in range(9, 36) for d in (-1, 0, 1)] +
                      [int(MIB * 1.07 ** k) for k in range(150)] + [7 * (1 << k) // 5 for k in range(10, 36)]))
    prev = 0
    for r in reqs:
        c = bb(r)
        assert c >= r and c >= prev and c % 512 == 0, (r, c, prev)
        assert bb(c) == c                                   # a class is its own class
        if r > MIB:
            assert (c - r) * 8 <= r, (r, c)                 # waste <= 12.5 % of the request
        else:
            assert c == max(512, 1 << (r - 1).bit_length())
        prev = c


def test_pool_header_parses_and_is_bound():
    names = declared_symbols("matinvent_hip_pool.h")
    assert names == sorted(["mi_pool_create", "mi_pool_destroy", "mi_pool_trim", "mi_pool_stats", "mi_pool_block_bytes", "mi_pool_set_poison",
                            "mi_batch_create_pooled", "mi_batch_index_table"])
    assert sorted(_lib.POOL_SIGNATURES) == names and any(t is _lib.POOL_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    build(verbose=False)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n


def test_handle_pool_config_parsing_and_refusals():
    from matinvent_amd.pool import parse_handle_pool
    assert parse_handle_pool(None) is None and parse_handle_pool(False) is None
    assert parse_handle_pool(True) == {}
    assert parse_handle_pool({}) == {} and parse_handle_pool({"max_bytes": None}) == {}
    assert parse_handle_pool({"max_bytes": 1 << 30}) == {"max_bytes": 1 << 30}
    for bad in ("yes", 1, 0, 2.5, [1], {"max_bytes": 0}, {"max_bytes": -4}, {"max_bytes": "1G"}, {"max_bytes": True}, {"max_bytes": 1.5},
                {"bytes": 4}, {"max_bytes": 8, "poison": True}):
        with pytest.raises(ValueError, match="handle_pool"):
            parse_handle_pool(bad)


def test_fit_refuses_a_bad_handle_pool_before_any_device_work():
    """fit parses cfg.handle_pool with its other keys: the refusal comes before the optimizer or a pool exists (the module here has no
    device behind it at all)."""
    from types import SimpleNamespace
    from matinvent_amd import pretrain
    m = SimpleNamespace(base=None)
    with pytest.raises(ValueError, match="handle_pool"):
        pretrain.fit(m, [object()], dict(lr=1e-3, epochs=1, batch_size=2, handle_pool="always"))


def test_creating_a_pool_without_a_gpu_is_the_librarys_error():
    import torch
    build(verbose=False)
    from matinvent_amd.pool import HandlePool
    if torch.cuda.is_available():   # (run on a GPU box: the same calls succeed)
        p = HandlePool()
        assert p.stats()["live_handles"] == 0 and p.stats()["bytes_reserved"] == 0
        p.close()
        return
    with pytest.raises(_lib.MIError) as ei:
        HandlePool()
    assert ei.value.code == _lib.MI_EHIP and "hipGetDevice" in str(ei.value)
    # and through the C entry itself: a code, a message, no handle
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.mi_pool_create(None, 0, C.byref(h)) == _lib.MI_EHIP and not h.value
    assert lib.mi_pool_create(None, 0, None) == _lib.MI_EINVAL
    assert lib.mi_pool_destroy(None) == 0 and lib.mi_pool_trim(None) == _lib.MI_EINVAL


def test_index_table_decode_on_the_host_matches_the_host_loops(tmp_path):
    """scripts/pool_tables_host_check.cpp: csrc/pool_tables.h -- what the kernels run per node, edge and pair -- against the literal
    loops of batch_create_impl, for every single crystal of 1 .. 200 atoms, [1, 7, 20, 3, 13] and 300 crystals cycling 1 .. 5."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "pool_tables_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "scripts", "pool_tables_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "204 cases, 0 mismatching" in r.stdout
