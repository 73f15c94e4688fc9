"""CPU-only tests of the multi-device MultiOutputGP_GPU surface: the device-list helper, the emulator split (the one of
dist.shard_bounds, empty blocks dropped) and the new C-ABI entries (declared, exported, prototyped)."""
import inspect
import os
import re

import numpy as np
import pytest

from mogp_emulator_amd import _capi, dist, fitting
from mogp_emulator_amd.devices import parse_devices, split_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mogp_mogp_create_on_devices", "mogp_mogp_n_parts", "mogp_mogp_part")


def test_all_and_lists():
    assert parse_devices("all", 4) == [0, 1, 2, 3]
    assert parse_devices(" ALL ", 2) == [0, 1]
    assert parse_devices([0, 0], 1) == [0, 0]
    assert parse_devices((3, 1), 4) == [3, 1]
    assert parse_devices(np.array([1, 0], dtype=np.int64), 2) == [1, 0]
    assert parse_devices("0, 1,1", 2) == [0, 1, 1]
    assert parse_devices([2], 3) == [2]


def test_environment_variable():
    assert parse_devices(None, 4, environ={}) is None
    assert parse_devices(None, 4, environ={"MOGP_DEVICES": "  "}) is None
    assert parse_devices(None, 4, environ={"MOGP_DEVICES": "all"}) == [0, 1, 2, 3]
    assert parse_devices(None, 4, environ={"MOGP_DEVICES": "0,0"}) == [0, 0]
    # an explicit list wins over the environment
    assert parse_devices([1], 4, environ={"MOGP_DEVICES": "all"}) == [1]
    with pytest.raises(ValueError):
        parse_devices(None, 4, environ={"MOGP_DEVICES": "0;1"})


@pytest.mark.parametrize("bad", [[-1], [4], [0, 4], [], "", "0,,1", "x", "1.5", [1.5], [True], ["0"], 3, "0,"])
def test_refusals(bad):
    with pytest.raises(ValueError):
        parse_devices(bad, 4)


def test_all_without_a_gpu_is_refused():
    with pytest.raises(ValueError):
        parse_devices("all", 0)


@pytest.mark.parametrize("n_items", [1, 2, 3, 5, 7, 8, 13, 64])
@pytest.mark.parametrize("n_dev", [1, 2, 3, 4, 8])
def test_split_is_shard_bounds_without_empty_blocks(n_items, n_dev):
    want = [(k,) + dist.shard_bounds(n_items, n_dev, k) for k in range(n_dev)]
    want = [w for w in want if w[1] < w[2]]
    assert split_bounds(n_items, n_dev) == want
    # contiguous and complete
    assert want[0][1] == 0 and want[-1][2] == n_items
    assert all(a[2] == b[1] for a, b in zip(want, want[1:]))


def test_two_emulators_on_three_devices_drop_the_empty_part():
    assert split_bounds(2, 3) == [(0, 0, 1), (1, 1, 2)]


def test_new_entries_are_declared_exported_and_prototyped():
    header = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1]
    res, args = _capi.SIGNATURES["mogp_mogp_create_on_devices"]
    assert len(args) == len(_capi.SIGNATURES["mogp_mogp_create"][1]) + 3


def test_create_on_devices_refuses_an_ordinal_outside_the_visible_range():
    """no device here is visible to the library or not -- either way an ordinal at the device count is out of range and the entry
    returns NULL with the library's message, before any device work"""
    lib = _capi.load()
    n = int(lib.mogp_device_count())
    X = np.zeros((4, 2))
    T = np.zeros((2, 4))
    dev = np.array([0, n], dtype=np.int32)
    h = lib.mogp_mogp_create_on_devices(_capi.dptr(X), 4, 2, _capi.dptr(T), 2, 10, None, 0, 0, 0., 0, _capi.iptr(dev), 2)
    assert not h
    assert "out of range" in _capi.last_error()
    h = lib.mogp_mogp_create_on_devices(_capi.dptr(X), 4, 2, _capi.dptr(T), 2, 10, None, 0, 0, 0., 0, None, 0)
    assert not h
    assert "at least one device" in _capi.last_error()


def test_python_surface_takes_devices():
    from mogp_emulator_amd import libgpgpu
    from mogp_emulator_amd.MultiOutputGP_GPU import MultiOutputGP_GPU
    assert "devices" in inspect.signature(MultiOutputGP_GPU.__init__).parameters
    assert "devices" in inspect.signature(libgpgpu.MultiOutputGP_GPU.__init__).parameters
    assert isinstance(MultiOutputGP_GPU.devices, property)
    assert "devices" in fitting._GP_KWARGS
