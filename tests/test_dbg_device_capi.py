"""mtg_boss_write_dbg_device at the C ABI, without a device: the export is declared and loadable, and
the argument checks come before anything touches the constructor or the GPU."""
import ctypes
import importlib
import os

import pytest

boss = importlib.import_module("projects2014-metagenome_amd.boss")

MTG_ERR_ARGUMENT = -5


def test_export_is_declared_and_loadable():
    assert "mtg_boss_write_dbg_device" in boss.EXPORTS
    fn = boss.lib().mtg_boss_write_dbg_device
    assert fn.argtypes is not None and len(fn.argtypes) == 9
    assert ctypes.sizeof(boss.DbgWriteTimings) == 32  # three doubles and a u64


def _chunk():
    # a descriptor that passes the pointer checks; nothing dereferences it in these calls
    c = boss._DeviceChunk(k=3, n=4)
    c.W = 4096
    c.last = 8192
    return c


@pytest.mark.parametrize("null", ["ctor", "chunk", "outbase"])
def test_null_arguments_are_refused(tmp_path, null):
    L = boss.lib()
    base = str(tmp_path / "g")
    # the checks run before the constructor is used, so a placeholder stands in where it is not the
    # NULL under test
    placeholder = ctypes.create_string_buffer(1 << 16)
    ctor = None if null == "ctor" else ctypes.cast(placeholder, ctypes.c_void_p)
    chunk = None if null == "chunk" else ctypes.byref(_chunk())
    outbase = None if null == "outbase" else os.fsencode(base)
    nv = ctypes.c_uint64(7)
    rc = L.mtg_boss_write_dbg_device(ctor, chunk, 0, outbase, 0, 0, -1, ctypes.byref(nv), None)
    assert rc == MTG_ERR_ARGUMENT
    assert b"write_dbg_device" in L.mtg_last_error()
    assert nv.value == 7
    assert os.listdir(str(tmp_path)) == []


def test_bad_modes_and_empty_chunk_are_refused_before_the_device(tmp_path):
    L = boss.lib()
    base = os.fsencode(str(tmp_path / "g"))
    placeholder = ctypes.create_string_buffer(1 << 16)
    ctor = ctypes.cast(placeholder, ctypes.c_void_p)
    good = dict(bits=0, mode=0, mask=0)
    for bad in (dict(mode=2), dict(mode=-1), dict(mask=3), dict(mask=-1), dict(bits=33)):
        a = dict(good, **bad)
        rc = L.mtg_boss_write_dbg_device(ctor, ctypes.byref(_chunk()), a["bits"], base, a["mode"], a["mask"],
                                         -1, None, None)
        assert rc == MTG_ERR_ARGUMENT, bad
    c = _chunk()
    c.n = 0
    assert L.mtg_boss_write_dbg_device(ctor, ctypes.byref(c), 0, base, 0, 0, -1, None, None) == MTG_ERR_ARGUMENT
    c = _chunk()
    c.W = None
    assert L.mtg_boss_write_dbg_device(ctor, ctypes.byref(c), 0, base, 0, 0, -1, None, None) == MTG_ERR_ARGUMENT
    assert os.listdir(str(tmp_path)) == []
