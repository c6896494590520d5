"""CPU side of the per-request sampling parameters (car_sampling_row, the four car_*_rows entries): the struct layout, the bound symbols, the argument
normalisation of Engine.generate / score / sample (sampling_rows) and dist.shard_rows."""
import ctypes as C
import os
import re

import pytest
import torch

from controlar_amd import _lib as L
from controlar_amd import dist
from controlar_amd.engine import Engine, sampling_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"car_generate_rows": 13, "car_generate_c2i_rows": 11, "car_score_rows": 13, "car_sample_logits_rows": 9}
KW = dict(cfg_scale=1.0, cfg_interval=-1, temperature=1.0, top_k=0, top_p=1.0, sample_logits=False, seed=0, control_strength=1.0)


def test_row_struct_layout():
    assert C.sizeof(L.CarSamplingRow) == 40
    want = {"cfg_scale": (0, C.c_float), "cfg_interval": (4, C.c_int32), "temperature": (8, C.c_float), "top_k": (12, C.c_int32),
            "top_p": (16, C.c_float), "sample_logits": (20, C.c_int32), "seed": (24, C.c_uint64), "control_strength": (32, C.c_float),
            "rng_stream": (36, C.c_uint32)}
    assert [n for n, _ in L.CarSamplingRow._fields_] == list(want)
    for name, typ in L.CarSamplingRow._fields_:
        assert (getattr(L.CarSamplingRow, name).offset, typ) == want[name], name
    assert C.sizeof(L.CarSampling) == 56                     # the call-wide struct is unchanged
    assert L.CAR_ABI_VERSION == 2                            # additive: the ABI version stays


def test_header_declares_the_struct_and_the_entries():
    hdr = open(os.path.join(ROOT, "include", "controlar_hip.h")).read()
    m = re.search(r"typedef struct car_sampling_row \{(.*?)\} car_sampling_row;", hdr, re.S)
    assert m
    fields = re.findall(r"^\s*(float|int32_t|uint32_t|uint64_t)\s+(\w+);", m.group(1), re.M)
    ctypes_of = {"float": C.c_float, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    assert [(n, ctypes_of[t]) for t, n in fields] == list(L.CarSamplingRow._fields_)
    for name, n in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n, (name, args)
        k = [i for i, a in enumerate(args) if "car_sampling_row" in a]
        assert len(k) == 1 and "car_sampling*" in args[k[0] - 1].replace(" ", "") and args[k[0]].startswith("const car_sampling_row*"), (name, args)
        plain = re.search(r"\bint\s+" + name[:-5] + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)          # the existing signature plus `rows` behind `sp`
        assert plain and len(plain.group(1).split(",")) == n - 1


def test_both_libraries_export_the_row_entries_with_the_declared_argument_counts():
    for path in (L.LIB_PATH, L.DEV_LIB_PATH):
        lib = C.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)
    for name, n in NEW.items():
        res, args = L.SYMBOLS[name]
        assert res is C.c_int and len(args) == n
        assert args.count(C.POINTER(L.CarSamplingRow)) == 1 and args[args.index(C.POINTER(L.CarSamplingRow)) - 1] == C.POINTER(L.CarSampling)
        plain = L.SYMBOLS[name[:-5]][1]
        assert [a for a in args if a != C.POINTER(L.CarSamplingRow)] == plain
    assert L.load().car_abi_version() == 2


def test_all_scalars_mean_the_existing_call():
    assert sampling_rows(4, None, **KW) is None
    assert sampling_rows(4, None, **dict(KW, cfg_scale=torch.tensor(3.0), seed=7)) is None          # a 0-d tensor is one value
    assert Engine.sampling_rows is sampling_rows


def test_scalars_are_broadcast_and_rng_stream_defaults_to_zero():
    rows = sampling_rows(3, None, **dict(KW, cfg_scale=4.0, temperature=[0.5, 1.0, 2.0], top_k=None, seed=torch.tensor([1, 2 ** 40 + 5, 3])))
    assert len(rows) == 3
    assert [r.temperature for r in rows] == [0.5, 1.0, 2.0]
    assert [r.seed for r in rows] == [1, 2 ** 40 + 5, 3]
    assert all(r.cfg_scale == 4.0 and r.cfg_interval == -1 and r.top_k == 0 and r.top_p == 1.0 and r.sample_logits == 0 for r in rows)
    assert all(r.control_strength == 1.0 and r.rng_stream == 0 for r in rows)
    # rng_stream alone selects the row call: one value for all, or one per image
    assert [r.rng_stream for r in sampling_rows(3, 5, **KW)] == [5, 5, 5]
    assert [r.rng_stream for r in sampling_rows(3, (0, 1, 2), **KW)] == [0, 1, 2]
    rows = sampling_rows(2, None, **dict(KW, sample_logits=(True, False), control_strength=torch.tensor([0.5, 2.0]), cfg_interval=[3, -1]))
    assert [(r.sample_logits, r.control_strength, r.cfg_interval) for r in rows] == [(1, 0.5, 3), (0, 2.0, -1)]


@pytest.mark.parametrize("name,val", [("temperature", [1.0, 2.0]), ("seed", torch.arange(4)), ("cfg_scale", (2.0,)), ("top_k", [])])
def test_length_mismatch_raises_before_the_library(name, val):
    with pytest.raises(ValueError, match=name):
        sampling_rows(3, None, **dict(KW, **{name: val}))


def test_rng_stream_length_mismatch_raises():
    with pytest.raises(ValueError, match="rng_stream"):
        sampling_rows(3, [0, 1], **KW)


def test_mixed_cfg_rows_raise():
    with pytest.raises(ValueError, match="call-wide"):
        sampling_rows(3, None, **dict(KW, cfg_scale=[1.5, 1.0, 3.0]))
    with pytest.raises(ValueError, match="call-wide"):
        sampling_rows(2, None, **dict(KW, cfg_scale=[0.5, 1.0 + 2 ** -20]))
    assert sampling_rows(2, None, **dict(KW, cfg_scale=[0.5, 1.0])) is not None          # all <= 1
    assert sampling_rows(2, None, **dict(KW, cfg_scale=[1.5, 7.5])) is not None          # all > 1


@pytest.mark.parametrize("G", [5, 8])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_shard_rows_agrees_with_shard_slice(G, world):
    params = dict(cfg_scale=[1.5 + i for i in range(G)], seed=torch.arange(100, 100 + G), top_k=tuple(range(G)), temperature=0.7, rng_stream=None)
    per = dist.pad_to_world(G, world) // world
    seen = []
    for rank in range(world):
        sl = dist.shard_slice(G, world, rank)
        got = dist.shard_rows(params, G, world, rank)
        own = list(range(G))[sl]
        seen += own
        assert got["temperature"] == 0.7 and got["rng_stream"] is None                   # one value for the call passes through
        for name in ("cfg_scale", "seed", "top_k"):
            full = params[name].tolist() if torch.is_tensor(params[name]) else list(params[name])
            vals = got[name].tolist() if torch.is_tensor(got[name]) else list(got[name])
            assert len(vals) == per                                                       # every rank decodes the same batch size
            assert vals[:len(own)] == full[sl]                                            # the rank's own requests, in shard_slice's order
            assert vals[len(own):] == [full[-1]] * (per - len(own))                       # pad entries repeat the last request
        assert type(got["top_k"]) is list and torch.is_tensor(got["seed"])
        assert sampling_rows(per, None, **dict(KW, **{k: v for k, v in got.items() if k != "rng_stream"})) is not None
    assert sorted(seen) == list(range(G))
    with pytest.raises(ValueError, match="cfg_scale"):
        dist.shard_rows(dict(cfg_scale=[1.0] * (G + 1)), G, world, 0)
