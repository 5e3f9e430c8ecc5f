"""The unitig entries at the C ABI, without a device: the exports are declared and loadable, the ctypes
structs have the header's layout, and the argument checks come before anything touches the constructor
or the GPU."""
import ctypes
import importlib
import os
import re

import pytest

boss = importlib.import_module("projects2014-metagenome_amd.boss")

MTG_ERR_UNSUPPORTED = -3
MTG_ERR_ARGUMENT = -5
NAMES = {"mtg_boss_unitigs_device": 5, "mtg_device_unitigs_free": 1, "mtg_boss_write_unitigs_device": 5,
         "mtg_boss_unitigs_last_rounds": 1}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtg_boss.h")


def test_exports_are_declared_and_loadable():
    header = open(HEADER).read()
    L = boss.lib()
    for name, nargs in NAMES.items():
        assert name in boss.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
        assert re.search(r"^(int|void|uint64_t) %s\(" % name, header, re.M), name
    version = int(re.search(r"#define MTG_BOSS_ABI_VERSION (\d+)", header).group(1))
    assert L.mtg_boss_abi_version() == version


def test_struct_layouts_match_the_header():
    header = open(HEADER).read()
    for cname, cls in (("mtg_unitig_params", boss._UnitigParams), ("mtg_device_unitigs", boss._DeviceUnitigs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*") for f in decl.split(None, 1)[1].split(",")]
        assert fields == [name for name, _ in cls._fields_], cname
    assert ctypes.sizeof(boss._UnitigParams) == 16
    assert ctypes.sizeof(boss._DeviceUnitigs) == 9 * 8  # 8 words and an int, padded
    assert boss._DeviceUnitigs.n_dropped_kmers.offset == 56 and boss._DeviceUnitigs.device_id.offset == 64


def _chunk(n=4, k=3):
    # a descriptor that passes the pointer checks; nothing dereferences it in these calls
    c = boss._DeviceChunk(k=k, n=n)
    c.W = 4096
    c.last = 8192
    return c


def _placeholder():
    # the checks run before the constructor is used, so a block of zeros stands in for it
    return ctypes.create_string_buffer(1 << 16)


@pytest.mark.parametrize("bad", ["ctor", "chunk", "out", "W", "last", "rows", "abundance", "huge"])
def test_unitigs_device_refuses_bad_arguments(bad):
    L = boss.lib()
    block = _placeholder()
    ctor = None if bad == "ctor" else ctypes.cast(block, ctypes.c_void_p)
    c = _chunk()
    if bad == "W":
        c.W = None
    if bad == "last":
        c.last = None
    if bad == "rows":
        c.n = 0
    if bad == "huge":
        c.n = 1 << 32
    p = boss._UnitigParams(1, 3 if bad == "abundance" else 1)
    out = boss._DeviceUnitigs(n_records=7)
    rc = L.mtg_boss_unitigs_device(ctor, None if bad == "chunk" else ctypes.byref(c), ctypes.byref(p), None,
                                   None if bad == "out" else ctypes.byref(out))
    assert rc == (MTG_ERR_UNSUPPORTED if bad == "huge" else MTG_ERR_ARGUMENT)
    assert b"unitigs_device" in L.mtg_last_error()
    if bad == "abundance":
        assert b"weights" in L.mtg_last_error()
    assert out.n_records == 7 and not out.seq


@pytest.mark.parametrize("bad", ["ctor", "chunk", "outbase", "abundance"])
def test_writer_refuses_bad_arguments_before_any_file(tmp_path, bad):
    L = boss.lib()
    block = _placeholder()
    ctor = None if bad == "ctor" else ctypes.cast(block, ctypes.c_void_p)
    c = _chunk()
    p = boss._UnitigParams(1, 2 if bad == "abundance" else 1)
    outbase = None if bad == "outbase" else os.fsencode(str(tmp_path / "u"))
    rc = L.mtg_boss_write_unitigs_device(ctor, None if bad == "chunk" else ctypes.byref(c), ctypes.byref(p), outbase,
                                         None)
    assert rc == MTG_ERR_ARGUMENT
    assert b"unitigs_device" in L.mtg_last_error()
    assert os.listdir(str(tmp_path)) == []


def test_free_of_an_empty_descriptor_is_harmless():
    L = boss.lib()
    u = boss._DeviceUnitigs()
    L.mtg_device_unitigs_free(ctypes.byref(u))
    L.mtg_device_unitigs_free(None)
    assert L.mtg_boss_unitigs_last_rounds(None) == 0
