"""ctypes binding of libd3h_hip.so (C ABI declared in include/d3h.h).

There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised
(the reference raises through TORCH_CHECK, render/renderutils/c_src/torch_bindings.cpp:27-31).

The binding is typed from d3h/_abi.py, the signature table tools/gen_header.py writes next to the header.  A symbol gets its `argtypes`
and `restype` from its row the first time it is looked up on the library object, so raw `lib().d3h_*` calls (bench.py, tests, tools) are
typed as well.  The package itself crosses the ABI through three functions only:
    call(name, *args)   entry points that return a status: converts and checks every argument against the row (tensor dtype, contiguity
                        and device for pointers, the C type's range for integers, the argument count), appends the current stream when the
                        row ends in `void* stream`, and raises RuntimeError on a non-zero code
    query(name, *args)  entry points that return a value (sizes, versions) -> int
    ptr_array(tensors)  a HOST array of device pointers for the `T* const*` parameters
`name` is the entry point without its `d3h_` prefix.  Every refusal happens before the native call.

`_use_emulator_for_tests(path)` exists only so that tests/test_emul_*.py can drive the very same Python
wrappers against tests/emul/libd3h_emul.so (the host emulation of the kernel sources used to debug kernel
logic in the GPU-less dev container).  Nothing in the package, bench.py or __graft_entry__ calls it.
"""
import ctypes
import os

import torch

from ._abi import ABI

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('D3H_LIB_PATH') or os.path.join(_HERE, 'libd3h_hip.so')     # D3H_LIB_PATH: A/B runs of two builds on one box
_lib = None
_emulated = False
ABI_VERSION = 7          # D3H_ABI_VERSION of include/d3h.h these wrappers were written against (csrc/d3h_common.h)

_I64 = ctypes.c_int64
_I32 = ctypes.c_int
_F32 = ctypes.c_float
_PTR = ctypes.c_void_p

# C scalar type -> (ctypes class, lowest, highest value); pointers are all c_void_p (it takes None, an address and any ctypes array)
_INTS = {'int': (_I32, -2**31, 2**31 - 1), 'unsigned': (ctypes.c_uint, 0, 2**32 - 1), 'int64_t': (_I64, -2**63, 2**63 - 1),
         'long long': (_I64, -2**63, 2**63 - 1), 'unsigned long long': (ctypes.c_uint64, 0, 2**64 - 1)}
_REALS = {'float': _F32, 'double': ctypes.c_double}
# pointee -> the tensor dtypes a pointer to it admits (None: any).  A `T* const*` parameter is a HOST array and admits no tensor.
_DTYPES = {'float': (torch.float32,), 'double': (torch.float64,), 'int': (torch.int32,), 'unsigned': (torch.int32,), 'int64_t': (torch.int64,), 'void': None,
           'unsigned long long': (torch.int64,),      # packed 64-bit keys (z | id, edge hash): opaque to torch, whose callers allocate int64
           'unsigned char': (torch.uint8,),           # flag / mask bytes: callers convert bool masks to uint8 before the call
           'uint8_t': (torch.uint8,)}                 # marching-tets case codes and `used` marks, allocated uint8
_INT_QUERIES = ('d3h_abi_version', 'd3h_topo_table_log2')        # int-valued results that are no status (next to every int64_t return)
_HOST = (ctypes.Array, ctypes._Pointer, _PTR, type(ctypes.byref(_I32())))      # the caller's own HOST memory (or a ptr_any() address): passed through


class _Lib(ctypes.CDLL):
    """the library with every symbol typed from the table on first use (CDLL caches the function object as an attribute); a library
    that lacks a symbol raises AttributeError only when that symbol is asked for"""

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        sig = ABI.get(name)
        if sig is not None:
            fn.restype = _INTS[sig[0]][0]
            fn.argtypes = [_PTR if t.endswith('*') else (_INTS.get(t) or (_REALS[t],))[0] for t, _ in sig[1]]
        return fn


def _load(path):
    l = _Lib(path)
    have = l.d3h_abi_version() if hasattr(l, 'd3h_abi_version') else None
    if have != ABI_VERSION:
        raise RuntimeError(f'd3h: the library reports ABI version {have}, these wrappers need {ABI_VERSION}: a stale build -- '
                           f'rebuild with __graft_entry__.build()')
    return l


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'd3h: {LIB_PATH} not built -- run __graft_entry__.build() '
                               f'(python d3human-code_amd/d3h/build.py); there is no CPU fallback')
        _lib = _load(LIB_PATH)
    return _lib


def _use_emulator_for_tests(path):
    """TEST ONLY (see module docstring)."""
    global _lib, _emulated
    _lib = _load(path)
    _emulated = True


def emulated():
    return _emulated


def _pointer_conv(where, pointee):
    dtypes = () if pointee.endswith('*') else _DTYPES[pointee]
    Tensor = torch.Tensor

    def conv(a):                     # (the order of the tests is the order of their frequency: this runs for every pointer of every call)
        if a is None:
            return None
        if isinstance(a, Tensor):
            if dtypes is not None and a.dtype not in dtypes:
                raise RuntimeError(f'd3h: {where}: a {pointee}* parameter takes ' + (' or '.join(str(d) for d in dtypes) or 'a HOST array') + f', got {a.dtype}')
            if not a.is_contiguous():
                raise RuntimeError(f'd3h: {where}: tensor must be contiguous')
            if not (a.is_cuda or _emulated):
                raise RuntimeError(f'd3h: {where}: tensors must live on the GPU (the product has no CPU path)')
            return a.data_ptr()
        if isinstance(a, _HOST):
            return a
        raise RuntimeError(f'd3h: {where}: expected a tensor, a ctypes array or None, got {type(a).__name__}')
    return conv


def _int_conv(where, ctype):
    _, lo, hi = _INTS[ctype]

    def conv(a):
        v = int(a)
        if not lo <= v <= hi:
            raise RuntimeError(f'd3h: {where}: {v} does not fit the parameter\'s type {ctype}')
        return v
    return conv


_bound = {}                  # entry point (without d3h_) -> (checked function, its argument count, has a stream, returns a value) ...
_bound_for = None            # ... looked up on this handle: another one (the emulation, a test's counting proxy) is bound afresh


def _bind(name):
    """-> the _bound row of d3h_<name> on the current library.  The row's function takes the arguments of call() / query(), converts each with
    its converter above and makes the native call.  It is generated, one expression per parameter, because the per-argument loop it
    replaces was the whole host cost of a call (tools/abi_call_cost.py): the common argument -- a plain tensor of the parameter's one dtype,
    an int in range -- is tested in line, everything else (None, a HOST array, a Parameter, a refusal) goes through the converter."""
    global _bound_for
    l = _lib or lib()
    if l is not _bound_for:
        _bound.clear()
        _bound_for = l
    if name in _bound:
        return _bound[name]
    sig = ABI.get('d3h_' + name)
    if sig is None:
        raise RuntimeError(f'd3h: {name} is no entry point of include/d3h.h')
    try:
        fn = getattr(l, 'd3h_' + name)
    except AttributeError:
        raise RuntimeError(f'd3h: the loaded library has no d3h_{name}') from None
    params = sig[1]
    has_stream = bool(params) and params[-1] == ('void*', 'stream')
    env, exprs = {'fn': fn, 'Tensor': torch.Tensor}, []
    for k, (ctype, pname) in enumerate(params[:-1] if has_stream else params):
        where, base = f'{name}({pname})', ctype.replace('const ', '').replace(' const', '')
        if base.endswith('*'):
            env[f'c{k}'], dtypes = _pointer_conv(where, base[:-1]), None if base.endswith('**') else _DTYPES[base[:-1]]
            if dtypes is not None and len(dtypes) == 1:
                env[f'd{k}'] = dtypes[0]
                exprs.append(f'(a{k}.data_ptr() if a{k}.__class__ is Tensor and a{k}.dtype is d{k} and a{k}.is_contiguous() and (a{k}.is_cuda or _emulated)'
                             f' else c{k}(a{k}))')
            else:
                exprs.append(f'c{k}(a{k})')
        elif base in _INTS:
            env[f'c{k}'] = _int_conv(where, base)
            exprs.append(f'(a{k} if a{k}.__class__ is int and {_INTS[base][1]} <= a{k} <= {_INTS[base][2]} else c{k}(a{k}))')
        else:
            exprs.append(f'float(a{k})')
    names = ', '.join(f'a{k}' for k in range(len(exprs)))
    src = f'def make({", ".join(env)}):\n def checked({names}):\n  return fn({", ".join(exprs + ["stream()"] * has_stream)})\n return checked\n'
    scope = {}
    exec(src, globals(), scope)
    b = _bound[name] = (scope['make'](**env), len(exprs), has_stream, sig[0] != 'int' or 'd3h_' + name in _INT_QUERIES)
    return b


def _refuse(name, row, nargs, value):
    _keepalive.clear()
    if row[3] != value:
        raise RuntimeError(f'd3h: {name} returns a ' + ('value: use query()' if row[3] else 'status: use call()'))
    raise RuntimeError(f'd3h: {name} takes {row[1]} arguments' + (' (and the stream, which call() adds)' if row[2] else '') + f', got {nargs}')


class StatusError(RuntimeError):
    """a non-zero status of an entry point; `code` for the few callers that give one code a message of their own"""

    def __init__(self, name, code):
        super().__init__(f'd3h: {name} failed with code {code}' + (' (bad argument)' if code < 0 else ' (hipError_t)'))
        self.code = code


def call(name, *args):
    """run the status-returning entry point d3h_<name>: arguments checked against its row of d3h/_abi.py (module docstring), the current
    stream appended where the entry point takes one; RuntimeError on a refusal (before the native call) or a non-zero status"""
    row = (_bound.get(name) if _lib is _bound_for else None) or _bind(name)
    if len(args) != row[1] or row[3]:
        _refuse(name, row, len(args), False)
    try:
        rc = row[0](*args)
    finally:
        if _keepalive:
            _keepalive.clear()
    if rc:
        raise StatusError(name, rc)


def query(name, *args):
    """the value (a size, a version) the entry point d3h_<name> returns, as an int; arguments checked as by call()"""
    row = (_bound.get(name) if _lib is _bound_for else None) or _bind(name)
    if len(args) != row[1] or not row[3]:
        _refuse(name, row, len(args), True)
    try:
        return int(row[0](*args))
    finally:
        _keepalive.clear()


_keepalive = []


def _address(t, dense=False, strided=False):
    if not (strided or t.is_contiguous() or dense and t.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError('d3h: tensor must be ' + ('dense (contiguous or channels-last)' if dense else 'contiguous'))
    if not _emulated and not t.is_cuda:
        raise RuntimeError('d3h: tensors must live on the GPU (the product has no CPU path)')
    return t.data_ptr()


def ptr(t):
    """device pointer of a contiguous tensor (None -> NULL), for raw `lib().d3h_*` calls (tests, tools).  The tensor is kept alive until
    the matching check() -- or the end of the call() the pointer goes into -- so that temporaries such as `ptr(g.contiguous())` cannot be
    freed (and their memory re-used) before the call is enqueued.  A tensor passed to call() itself needs none of this: the argument
    tuple holds it for the duration of the call."""
    if t is None:
        return None
    p = _PTR(_address(t))
    _keepalive.append(t)
    return p


def ptr_any(t):
    """device pointer of a DENSE tensor in whatever memory format it has (contiguous or channels-last): the callee is told the layout"""
    if t is None:
        return None
    p = _PTR(_address(t, dense=True))
    _keepalive.append(t)
    return p


def ptr_array(tensors, strided=False):
    """HOST array of the device pointers of contiguous tensors (None -> NULL) for a `T* const*` parameter; the array holds the tensors,
    so temporaries among them live as long as it does.  `strided`: slices of pixel-major tensors, whose pitch the callee is told."""
    a = (_PTR * len(tensors))(*[None if t is None else _address(t, strided=strided) for t in tensors])
    a.tensors = tensors
    return a


def stream():
    """the raw handle of torch's current stream on the current device.  NOT torch.cuda.current_stream(): that goes through
    torch.cuda.is_available() -> an environment lookup and a device-count query of the runtime on EVERY call -- ~120 us each on this
    stack, 34 calls = 4 ms of host time per 7.6 ms training iteration (tools/gpu_cpu_profile.py), which had become the bottleneck of
    the step once the GPU work had shrunk below the host's launch loop."""
    if _emulated:
        return None
    return _PTR(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def cur_stream():
    """torch.cuda.current_stream() without its per-call availability probe (see stream()): passing the device index takes the fast path"""
    return torch.cuda.current_stream(torch._C._cuda_getDevice())


class use_stream:
    """`with torch.cuda.stream(s)` without its `torch.cuda.current_stream(None)` (the slow availability-probing path, see stream()): the
    previous stream comes from cur_stream() and both switches go straight to the binding -- ~5 us instead of ~80 per use"""
    __slots__ = ('s', 'prev')

    def __init__(self, s):
        self.s = s

    def __enter__(self):
        self.prev = cur_stream()
        s = self.s
        torch._C._cuda_setStream(stream_id=s.stream_id, device_index=s.device_index, device_type=s.device_type)
        return s

    def __exit__(self, *exc):
        p = self.prev
        torch._C._cuda_setStream(stream_id=p.stream_id, device_index=p.device_index, device_type=p.device_type)
        return False


# ---- zero-filled tensors without a fill launch each ---------------------------------------------------------------------------------
# A config-3 step asked torch for ~20 zero-filled tensors (gradient accumulators of the atomic-scatter kernels, padded index lists): ~20 fill
# kernels of ~5 us on the launch-bound parts of the step (profiles/r5_bench_config3_per_iteration_serialised.csv: FillFunctor x 20).  zeros() carves
# them from a slab that ONE fill zeroed: 32 MB per (device, stream) -- the same stream semantics as torch.zeros, whose fill also runs on the
# current stream -- replaced by a fresh one when used up (never re-used: a carved tensor keeps its slab alive, like a view its base).  The carved
# tensors are not views (Tensor.set_ on the slab's storage): each has its own autograd version counter, so an in-place op on one cannot
# invalidate another that an autograd node saved.  D3H_ZERO_SLAB=0: plain torch.zeros.
# (a tensor that escapes -- a gradient adopted as `.grad`, a ctx buffer of a retained graph -- pins its whole slab, and torch.save of such a
# tensor would serialise the slab's storage: checkpoints are written from parameters and optimiser state, never from `.grad`
# (d3h/checkpoint.py).  The slab stays at 32 MB because the step carves pieces of 3.1 MB (d(grid positions)) and 4.3 MB (the texture tables'
# gradient) from it -- a quarter of a smaller slab would send them back to one fill launch each.  The per-stream table now evicts the least
# recently used entry instead of dropping every stream's live slab.)
ZERO_SLAB = os.environ.get('D3H_ZERO_SLAB', '1') != '0'
SLAB_BYTES = 32 << 20
import collections as _collections          # noqa: E402
_slabs = _collections.OrderedDict()
_ITEM = {}
SLAB_STATS = {'carved': 0, 'slabs': 0, 'plain': 0}


def zeros(shape, dtype=torch.float32, device=None):
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(v) for v in shape)
    dev = torch.device(device) if device is not None else torch.device('cpu')
    n = 1
    for v in shape:
        n *= v
    item = _ITEM.get(dtype)
    if item is None:
        item = _ITEM[dtype] = torch.empty(0, dtype=dtype).element_size()
    nbytes = n * item
    if not ZERO_SLAB or _emulated or dev.type != 'cuda' or nbytes == 0 or nbytes > SLAB_BYTES // 4:
        SLAB_STATS['plain'] += 1
        return torch.zeros(shape, dtype=dtype, device=dev)
    idx = dev.index if dev.index is not None else torch._C._cuda_getDevice()
    key = (idx, torch._C._cuda_getCurrentRawStream(idx))
    slab = _slabs.get(key)
    if slab is not None:
        _slabs.move_to_end(key)
    off = 0 if slab is None else (slab[1] + 255) & ~255
    if slab is None or off + nbytes > SLAB_BYTES:
        if slab is None and len(_slabs) >= 16:         # streams come and go (tests): do not keep a slab per stream handle ever seen
            _slabs.popitem(last=False)
        slab = _slabs[key] = [torch.zeros(SLAB_BYTES, dtype=torch.uint8, device=torch.device('cuda', idx)), 0]
        SLAB_STATS['slabs'] += 1
        off = 0
    t = torch.empty(0, dtype=dtype, device=slab[0].device).set_(slab[0].untyped_storage(), off // item, shape)
    slab[1] = off + nbytes
    SLAB_STATS['carved'] += 1
    return t


def zeros_like(t, dtype=None):
    return zeros(t.shape, dtype or t.dtype, t.device)


def check(rc, what):
    _keepalive.clear()
    if rc != 0:
        raise StatusError(what, rc)


def i64(v):
    return _I64(int(v))


def i32(v):
    return _I32(int(v))


def f32(v):
    return _F32(float(v))
