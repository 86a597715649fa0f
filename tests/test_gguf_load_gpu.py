"""The GGUF load entries against a recorded fixture: tests/golden/gguf_load/manifest.txt holds, for seeded blocks of
every type at the smallest shapes with padding (tools/gguf_load_digest.py), the SHA-256 of the device layout bytes and
of the fp32 unpack, the 14 values of nad_weight_info2, and nad_device_get_compute / the M = 1 plan in int8 mode (which
pins the activation quantizer of the type).  The manifest was written by the library of the commit named in its first
line; a later library must reproduce it exactly -- the layout bytes did not change -- so nothing here has a tolerance.
Every load goes through the C entries onto a buffer with 256 guard bytes behind it.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gguf_load_digest", os.path.join(REPO, "tools", "gguf_load_digest.py"))
dig = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dig)

if gpu_available():
    import torch
    from neural_amd import _lib, bestla

NAMES = list(dig.TYPES)
_RECORDS = {}


def _blocks(name):
    return np.fromfile(dig.blocks_path(name), np.uint8)


def _record(name):
    """the type's blocks loaded through its own entry, once"""
    if name not in _RECORDS:
        _RECORDS[name] = dig.record(name, _blocks(name))
    return _RECORDS[name]


@pytest.fixture(scope="module")
def manifest():
    return dig.read_manifest()


def test_fixture_blocks_are_the_seeded_ones():
    for name in NAMES:
        tid, be, bb, _, _, n, k = dig.TYPES[name]
        blocks = _blocks(name)
        assert blocks.size == n * (k // be) * bb
        assert np.array_equal(blocks, dig.make_blocks(name))


@pytest.mark.parametrize("name", NAMES)
def test_load_reproduces_the_recorded_layout(manifest, name):
    r = _record(name)
    line = dig.manifest_line(name, r)
    print(line)
    assert (r["guard"] == dig.FILL).all(), "the load wrote past the bytes its size entry asks for"
    assert line == manifest[name]


def test_q4_0_through_both_entries_is_the_same_weight():
    L = _lib.lib()
    a = _record("q4_0")
    b = dig.record("q4_0", _blocks("q4_0"), entry=(lambda n, k: L.nad_gguf_device_size(2, n, k),
                                                   lambda *args: L.nad_gguf_device_load(2, *args)))
    assert a["need"] == b["need"]
    assert np.array_equal(a["layout"], b["layout"]) and (b["guard"] == dig.FILL).all()
    assert a["info"] == b["info"] and a["compute"] == b["compute"] and a["plan"] == b["plan"]
    assert np.array_equal(a["unpack"].view(np.uint32), b["unpack"].view(np.uint32))


ENTRIES = [("nad_q4_0_device_load", "q4_0", None), ("nad_q6_k_device_load", "q6_k", None)] + \
          [("nad_gguf_device_load", name, dig.TYPES[name][0]) for name in NAMES if name != "q6_k"]


@pytest.mark.parametrize("entry,name,tid", ENTRIES, ids=[f"{e}-{n}" for e, n, _ in ENTRIES])
def test_short_buffer_is_refused_by_name_and_devstor_untouched(entry, name, tid):
    L = _lib.lib()
    n, k = dig.TYPES[name][5:7]
    blocks = _blocks(name)
    need = dig.entries(L, name)[0](n, k)
    mem = torch.full((need + dig.GUARD,), dig.FILL, dtype=torch.uint8, device="cuda")
    desc = (C.c_uint8 * L.bestla_device_storage_size())(*([0x5A] * L.bestla_device_storage_size()))
    args = (bestla._ptr(blocks), n, k, desc, bestla._ptr(mem), need - 1, bestla._stream())
    L.nad_clear_error()
    rc = getattr(L, entry)(*((tid,) + args if tid is not None else args))
    torch.cuda.synchronize()
    assert rc == -1
    assert entry in _lib.last_error(), _lib.last_error()
    assert bytes(desc) == bytes([0x5A]) * len(desc)
    assert bool((mem == dig.FILL).all())
    L.nad_clear_error()
