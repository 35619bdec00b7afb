"""The C-ABI library builds for gfx950 (hipcc cross-compiles without a GPU), loads, and exports every symbol include/d3h.h
declares.  No compute calls here (no GPU in the dev container)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'd3h.h')).read()
    return sorted(set(re.findall(r'\b(d3h_[a-z0-9_]+)\s*\(', txt)))


def test_header_is_valid_c():
    subprocess.check_call(['gcc', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'd3h.h')])


def test_library_builds_and_exports_every_declared_symbol():
    from d3h import build as B
    so = B.build(verbose=False)
    lib = ctypes.CDLL(so)
    names = _declared()
    assert len(names) >= 38
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_every_exported_entry_point_is_declared():
    """no source file is left out of the generated header"""
    import glob
    defined = set()
    for f in glob.glob(os.path.join(ROOT, 'd3human-code_amd', 'csrc', '*.hip')):
        src = open(f).read()
        defined |= set(re.findall(r'extern "C" [^{;]*?\b(d3h_[a-z0-9_]+)\s*\(', src))
        defined |= set(re.findall(r'#define d3h_sdf_mlp\w+ (d3h_deform_mlp\w+)', src))      # renamed second build of the MLP sources
    assert defined and defined == set(_declared()), sorted(defined ^ set(_declared()))


def test_header_matches_sources():
    """include/d3h.h is generated from the extern "C" definitions: regenerate and compare"""
    before = open(os.path.join(ROOT, 'include', 'd3h.h')).read()
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'gen_header.py')], stdout=subprocess.DEVNULL)
    assert open(os.path.join(ROOT, 'include', 'd3h.h')).read() == before


def test_product_refuses_cpu_tensors():
    """the product has no CPU path: the ctypes layer rejects host tensors unless the test-only emulator hook is active"""
    import pytest
    import torch
    from d3h import _lib as L
    L._lib, L._emulated = None, False
    with pytest.raises(RuntimeError):
        L.ptr(torch.zeros(4))
    assert not L._keepalive


# ---- the signature table (d3h/_abi.py) and the typed binding (d3h/_lib.py: call / query / ptr_array) ----------------------------------

def _header_arity():
    """{name: parameter count} of every declaration in include/d3h.h"""
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'd3h.h')).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r'\b(d3h_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', txt):
        n = 0 if params.strip() in ('', 'void') else params.count(',') + 1
        assert out.setdefault(name, n) == n, name
    return out


def test_abi_table_matches_header():
    """d3h/_abi.py is generated with the header: regenerating is a no-op, its names are the header's, each row has the header's arity"""
    path = os.path.join(ROOT, 'd3human-code_amd', 'd3h', '_abi.py')
    before = open(path).read()
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'gen_header.py')], stdout=subprocess.DEVNULL)
    assert open(path).read() == before
    from d3h._abi import ABI
    assert sorted(ABI) == _declared()
    assert {k: len(v[1]) for k, v in ABI.items()} == _header_arity()
    assert all(n for _, row in ABI.values() for _, n in row), 'a parameter without a name'


def _unreachable(L, monkeypatch, name):
    """replace the library's d3h_<name> by a function that fails the test if a refused call reaches it"""
    import pytest
    assert L.query('abi_version') == L.ABI_VERSION              # the binding now belongs to this library handle
    monkeypatch.setattr(L.lib(), 'd3h_' + name, lambda *a: pytest.fail(f'd3h_{name} was called'))
    monkeypatch.delitem(L._bound, name, raising=False)              # bound again, on the patched function


def _hash_args(torch, **over):
    a = dict(tri=torch.zeros(4, 3, dtype=torch.int32), nf=4, keys=torch.zeros(1024, dtype=torch.int64),
             vals=torch.zeros(2048, dtype=torch.int32), cap=1024)
    a.update(over)
    return list(a.values())


def test_call_refuses_before_the_native_call(emul, monkeypatch):
    import pytest
    import torch
    from d3h import _lib as L
    _unreachable(L, monkeypatch, 'antialias_hash')
    _unreachable(L, monkeypatch, 'env_shade_fwd')
    _unreachable(L, monkeypatch, 'relu6_bwd')
    cases = [
        (r'antialias_hash\(tri\).*int32.*int64', 'antialias_hash', _hash_args(torch, tri=torch.zeros(4, 3, dtype=torch.int64))),
        (r'relu6_bwd\(g\).*float32.*float64', 'relu6_bwd', [torch.zeros(4), torch.zeros(4, dtype=torch.float64), 4, torch.zeros(4)]),
        (r'antialias_hash\(tri\).*must be contiguous', 'antialias_hash', _hash_args(torch, tri=torch.zeros(3, 4, dtype=torch.int32).t())),
        (r'antialias_hash\(nf\).*2147483648', 'antialias_hash', _hash_args(torch, nf=2**31)),
        (r'antialias_hash takes 5 arguments.*got 4', 'antialias_hash', _hash_args(torch)[:-1]),
        (r'antialias_hash takes 5 arguments.*got 6', 'antialias_hash', _hash_args(torch) + [None]),
        (r'antialias_hash\(vals\).*expected a tensor', 'antialias_hash', _hash_args(torch, vals=7)),
    ]
    n_env = len(L.ABI['d3h_env_shade_fwd'][1]) - 1
    seed = [k for k, (t, n) in enumerate(L.ABI['d3h_env_shade_fwd'][1]) if n == 'seed'][0]
    assert L.ABI['d3h_env_shade_fwd'][1][seed][0] == 'unsigned'
    env = [None] * n_env
    for k, (t, _) in enumerate(L.ABI['d3h_env_shade_fwd'][1][:-1]):
        if not t.endswith('*'):
            env[k] = 0
    env[seed] = -1
    cases.append((r'env_shade_fwd\(seed\).*-1', 'env_shade_fwd', env))
    for match, name, args in cases:
        with pytest.raises(RuntimeError, match=match):
            L.call(name, *args)
        assert not L._keepalive, match
    # a pointer from ptr_any() is pinned until the call it goes into ends, refused or not
    with pytest.raises(RuntimeError):
        L.call('antialias_hash', *_hash_args(torch, keys=L.ptr_any(torch.zeros(1024, dtype=torch.int64)), nf=2**31))
    assert not L._keepalive
    with pytest.raises(RuntimeError, match='returns a value'):
        L.call('sdf_mlp_wpack_floats')
    with pytest.raises(RuntimeError, match='returns a status'):
        L.query('antialias_hash', *_hash_args(torch))


def test_call_refuses_host_tensors_without_the_emulator_hook(emul, monkeypatch):
    import pytest
    import torch
    from d3h import _lib as L
    _unreachable(L, monkeypatch, 'antialias_hash')
    monkeypatch.setattr(L, '_emulated', False)
    with pytest.raises(RuntimeError, match=r'antialias_hash\(tri\).*must live on the GPU'):
        L.call('antialias_hash', *_hash_args(torch))
    assert not L._keepalive


def test_call_accepts_none_ctypes_arrays_and_int32_for_unsigned(emul):
    import torch
    from d3h import _lib as L
    # None for a pointer (d_x of the backward the caller does not need) and n = 0: returns before any kernel
    assert L.ABI['d3h_relu6_bwd'][1][3] == ('float*', 'gx')
    L.call('relu6_bwd', torch.zeros(4), torch.zeros(4), 0, None)
    # a ctypes array for a pointer: the HOST result array of bvh_layout
    sizes = (ctypes.c_int64 * 4)()
    L.call('bvh_layout', 100, sizes)
    assert sizes[0] > 0
    # an int32 tensor for `const unsigned*` (the packed bf16 weight planes), n = 0
    sig = L.ABI['d3h_sdf_mlp_fwd_x3'][1]
    assert sig[3] == ('const unsigned*', 'wpack3')
    wp3 = torch.zeros(L.query('sdf_mlp_wpack3_dwords'), dtype=torch.int32)
    L.call('sdf_mlp_fwd_x3', torch.zeros(0, 3), None, 0.0, wp3, torch.zeros(0), None, None, 0, 0)
    assert L.query('abi_version') == L.ABI_VERSION and not L._keepalive
    # raw access is typed from the same table (bench.py reads the timing records this way)
    assert L.lib().d3h_timing_read.restype is ctypes.c_int64
    assert L.lib().d3h_timing_read(None, None, None, ctypes.c_int64(0)) == 0
    assert L.lib().d3h_timing_select(ctypes.c_uint64(1)) == 0 and L.lib().d3h_timing_enable(0) == 0 and L.lib().d3h_timing_reserve(ctypes.c_int64(0)) == 0


@pytest.mark.gpu
def test_gpu_call_refuses_int64_for_int_pointer(gpu, monkeypatch):
    """the dtype refusal with device tensors: nothing is launched"""
    import pytest
    import torch
    from d3h import _lib as L
    _unreachable(L, monkeypatch, 'antialias_hash')
    args = [a.cuda() if isinstance(a, torch.Tensor) else a for a in _hash_args(torch, tri=torch.zeros(4, 3, dtype=torch.int64))]
    with pytest.raises(RuntimeError, match=r'antialias_hash\(tri\).*int32.*int64'):
        L.call('antialias_hash', *args)
    assert not L._keepalive
