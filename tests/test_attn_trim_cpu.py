"""The lane predicates of the bf16 decode attention's edge blocks (decode2_params.h attn2_edge_k_lane / attn2_edge_v_lane, seen through the host-only
car_debug_attn_edge_mask) against a brute force over the packed KV layout.  The brute force below restates the WRITER's index formulas
(decode2.hip prefill_rope_kv2_kernel, the `kp` / `vp` lines): element (position t, dim d) of a 32-position block lands in load instruction i, lane l.
A lane must load if it holds an attended row (safety: otherwise an attended K / V element would read as zero) and must not load if it holds none
(tightness: that is the traffic the trim removes)."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from controlar_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _k_slot(t, d):
    """bf16 element offset inside a block of K -> (load instruction, lane): kp = ((t>>4)*2 + (d>>5))*512 + ((((d&31)>>3)*16 + (t&15))<<3) + (d&7)"""
    off = ((t >> 4) * 2 + (d >> 5)) * 512 + ((((d & 31) >> 3) * 16 + (t & 15)) << 3) + (d & 7)
    return off // 512, (off % 512) // 8


def _v_slot(t, d):
    """vp = ((t>>5)*4 + (d>>4))*512 + ((qv*16 + (d&15))<<3) + ev with w = t&31, (qv, ev) = w < 16 ? (w>>2, w&3) : ((w-16)>>2, 4 + ((w-16)&3))"""
    w = t & 31
    qv, ev = (w >> 2, w & 3) if w < 16 else ((w - 16) >> 2, 4 + ((w - 16) & 3))
    off = ((t >> 5) * 4 + (d >> 4)) * 512 + ((qv * 16 + (d & 15)) << 3) + ev
    return off // 512, (off % 512) // 8


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def holders():
    """[4*64] sets: the block positions whose elements sit in (instruction, lane), for K and for V; every slot of the 4 x 64 x 8 elements is hit exactly once"""
    k = [set() for _ in range(256)]
    v = [set() for _ in range(256)]
    nk, nv = np.zeros(256, int), np.zeros(256, int)
    for t in range(32):
        for d in range(64):
            i, l = _k_slot(t, d); k[i * 64 + l].add(t); nk[i * 64 + l] += 1
            i, l = _v_slot(t, d); v[i * 64 + l].add(t); nv[i * 64 + l] += 1
    assert (nk == 8).all() and (nv == 8).all()      # the formulas are bijections onto the block's 4 x 1 KiB
    return k, v


def _mask(lib, lo, hi):
    km, vm = np.full(256, 7, np.uint8), np.full(256, 7, np.uint8)
    assert lib.car_debug_attn_edge_mask(lo, hi, C.c_void_p(km.ctypes.data), C.c_void_p(vm.ctypes.data)) == 0
    return km, vm


def test_every_edge_range_is_safe_and_tight(lib, holders):
    kh, vh = holders
    for lo in range(32):
        for hi in range(lo, 32):
            att = set(range(lo, hi + 1))
            km, vm = _mask(lib, lo, hi)
            assert set(np.unique(km)) <= {0, 1} and set(np.unique(vm)) <= {0, 1}
            for s in range(256):
                assert km[s] == (1 if kh[s] & att else 0), ("K", lo, hi, s // 64, s % 64)
                assert vm[s] == (1 if vh[s] & att else 0), ("V", lo, hi, s // 64, s % 64)


def test_a_whole_block_loads_every_lane(lib):
    km, vm = _mask(lib, 0, 31)
    assert km.all() and vm.all()


def test_rows_fetched_match_the_line_arithmetic(lib):
    """K is skipped at 8-position granularity (a 128-byte line is 8 consecutive positions of 8 dims), V only where both quartets of a lane group are out
    of range — the figures DESIGN §4.1 quotes for the traffic"""
    for lo, hi in ((0, 0), (5, 5), (13, 31), (0, 7), (8, 15), (20, 27), (31, 31)):
        km, vm = _mask(lib, lo, hi)
        octets = len({t >> 3 for t in range(lo, hi + 1)})
        groups = len({(t & 15) >> 2 for t in range(lo, hi + 1)})
        assert km.sum() == (hi - lo + 1) * 8       # the K predicate is exact per position: (2 dim halves x 4 chunks) lanes each
        lines = km.reshape(32, 8).any(axis=1)      # a 128-byte line = 8 consecutive lanes of one load: what the memory system fetches
        assert lines.sum() == octets * 8           # whole octets: 8 lines = 8 rows' worth of bytes per octet touched
        assert vm.sum() == groups * 16 * 4         # 16 lanes x 4 instructions per lane group


def test_bad_ranges_are_refused(lib):
    km, vm = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    for lo, hi in ((-1, 3), (0, 32), (5, 4)):
        assert lib.car_debug_attn_edge_mask(lo, hi, C.c_void_p(km.ctypes.data), C.c_void_p(vm.ctypes.data)) != 0
    assert lib.car_debug_attn_edge_mask(0, 31, None, C.c_void_p(vm.ctypes.data)) != 0


def test_declared_in_the_header_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    assert re.search(r"int\s+car_debug_attn_edge_mask\s*\(\s*int32_t\s+lo\s*,\s*int32_t\s+hi\s*,", hdr)
    assert "car_debug_attn_edge_mask" in L.SYMBOLS


def test_the_switch_exists_only_in_the_development_library():
    rel = open(L.LIB_PATH, "rb").read()
    dev = open(L.DEV_LIB_PATH, "rb").read()
    assert b"CAR_ATTN_NO_TRIM" in dev and b"CAR_ATTN_NO_TRIM" not in rel
