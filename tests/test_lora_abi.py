"""CPU: the C ABI of the LoRa bank (include/sdrx.h, sdrx_lora_*): the symbols, the ctypes face against the header's structs, and
what create refuses before it touches a device."""
import ctypes as C
import os
import re

import pytest

import sdrangel_amd as sa

EINVAL = -1          # SDRX_EINVAL
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrx.h")
NAMES = ["create", "destroy", "reset", "feed", "feed_dev", "feed_bank", "sync", "set_stream", "get_stream", "set_timing", "get_timing", "last_launch",
         "read", "last_dev", "read_text", "state", "get_design"]


def test_symbols_exist_and_are_declared():
    lib = sa.lib()
    declared = sa.exported_symbols()
    for n in NAMES:
        assert hasattr(lib, "sdrx_lora_" + n), n
        assert "sdrx_lora_" + n in declared, n
    assert sorted(s for s in declared if s.startswith("sdrx_lora_")) == sorted("sdrx_lora_" + n for n in NAMES)


def _struct_fields(name):
    txt = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        out += [(ctype, n.strip()) for n in names.split(",")]
    return out


@pytest.mark.parametrize("cname,cls", [("sdrx_lora_cfg", sa.LoraCfg), ("sdrx_lora_state_t", sa.LoraState)])
def test_struct_layout_matches_the_header(cname, cls):
    sizes = {"int32_t": (4, C.c_int32), "int64_t": (8, C.c_int64)}
    fields = _struct_fields(cname)
    assert [n for _, n in fields] == [n for n, _ in cls._fields_]
    assert [sizes[t][1] for t, _ in fields] == [t for _, t in cls._fields_]
    off = 0
    for t, n in fields:                                    # natural alignment, as the C compiler lays it out
        size = sizes[t][0]
        off = (off + size - 1) // size * size
        assert getattr(cls, n).offset == off, n
        off += size
    assert C.sizeof(cls) == (off + 7) // 8 * 8 if any(t == "int64_t" for t, _ in fields) else C.sizeof(cls) == off


def _create(n_ch, cfgs, out=True):
    h = C.c_void_p()
    arr = (sa.LoraCfg * max(len(cfgs), 1))(*cfgs) if cfgs is not None else None
    rc = sa.lib().sdrx_lora_create(C.byref(h) if out else None, 0, n_ch, arr)
    return rc, sa.lib().sdrx_last_error().decode(), h


@pytest.mark.parametrize("n_ch,cfgs,out", [
    (1, [sa.LoraCfg(48000, 0, 0)], True),
    (1, [sa.LoraCfg(48000, 0, -7813)], True),
    (1, [sa.LoraCfg(7813, 0, 15625)], True),
    (2, [sa.LoraCfg(48000, 0, 7813), sa.LoraCfg(48000, 0, 48001)], True),
    (1, [sa.LoraCfg(0, 0, 7813)], True),
    (0, [sa.LoraCfg(48000, 0, 7813)], True),
    (-1, [sa.LoraCfg(48000, 0, 7813)], True),
    (1, None, True),
    (1, [sa.LoraCfg(48000, 0, 7813)], False),
])
def test_create_refuses_bad_arguments(n_ch, cfgs, out):
    rc, err, h = _create(n_ch, cfgs, out)
    assert rc == EINVAL and err.startswith("sdrx_lora_create") and not h.value


def test_null_handles_are_refused():
    lib = sa.lib()
    assert lib.sdrx_lora_destroy(None) == 0
    for name, args in (("reset", []), ("feed", [None, None]), ("feed_dev", [None, None]), ("feed_bank", [None]), ("sync", []), ("state", [0, None])):
        assert getattr(lib, "sdrx_lora_" + name)(None, *args) == EINVAL, name
    assert lib.sdrx_lora_read(None, 0, None, 0) == EINVAL and lib.sdrx_lora_read_text(None, 0, None, 0) == EINVAL
