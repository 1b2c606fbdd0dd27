"""ctypes binding of libmvsdf_hip.so (C ABI: include/mvsdf_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, we raise.
"""
import ctypes as C
import os
import re
import struct

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get('MVSDF_LIB') or os.path.join(_HERE, 'libmvsdf_hip.so')   # MVSDF_LIB: dev override (ablation builds)
MAX_LAYERS = 12
_lib = None


class NetDesc(C.Structure):
    _fields_ = [('n_layers', C.c_int), ('K', C.c_int * MAX_LAYERS), ('N', C.c_int * MAX_LAYERS),
                ('wp', C.c_void_p * MAX_LAYERS), ('bias', C.c_void_p * MAX_LAYERS), ('w', C.c_void_p * MAX_LAYERS),
                ('skip_layer', C.c_int), ('multires', C.c_int), ('wp16', C.c_void_p * MAX_LAYERS), ('trace_dtype', C.c_int), ('skip_mask', C.c_uint), ('wx3', C.c_void_p * MAX_LAYERS)]


class TraceParams(C.Structure):
    _fields_ = [('r', C.c_float), ('thr', C.c_float), ('line_search_step', C.c_float), ('line_step_iters', C.c_int),
                ('st_iters', C.c_int), ('n_steps', C.c_int), ('n_secant', C.c_int), ('dist_clip', C.c_float)]


class MvsdfError(RuntimeError):
    pass


def lib():
    """Load the HIP library (built in-tree by mvsdf_amd/build.py).  Raises if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise MvsdfError('libmvsdf_hip.so not found at %s -- run `python -c "import __graft_entry__ as g; g.build()"` '
                             '(hipcc --offload-arch=gfx950); there is no CPU/PyTorch fallback for the hot path' % SO_PATH)
        import torch  # noqa: F401  -- load torch's bundled HIP runtime first so this library binds to the same libamdhip64
        L = C.CDLL(SO_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


# ---- the prototypes: derived from the header every .hip file is compiled against, so the compiler checks the definitions and this checks the calls
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'mvsdf_hip.h')
# every by-value spelling the header may use; anything else is an error, never a guess
_SCALARS = {'int': C.c_int, 'unsigned': C.c_uint, 'unsigned int': C.c_uint, 'long long': C.c_longlong, 'unsigned long long': C.c_ulonglong,
            'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'size_t': C.c_size_t,
            'float': C.c_float, 'double': C.c_double}


def _ctype(spelling, fn, named):
    """ctypes type of one parameter (`named`: a last word that completes no known type is the parameter's name) or return type.  Pointers and arrays are
    c_void_p: byref(), ctypes arrays, None, data_ptr() ints and c_void_p instances all pass."""
    if '*' in spelling or '[' in spelling:
        return C.c_void_p
    words = [w for w in spelling.split() if w != 'const']
    if named and len(words) > 1 and ' '.join(words) not in _SCALARS:
        words = words[:-1]
    try:
        return _SCALARS[' '.join(words)]
    except KeyError:
        raise MvsdfError('%s: no ctypes mapping for the C type "%s"' % (fn, ' '.join(words))) from None


def parse_header(text):
    """{name: (restype, [argtypes])} of every `ret mvsdf_name(args);` declaration of a C header, in its order."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', ' ', text, flags=re.M)                # preprocessor lines with their continuations
    protos = {}
    for ret, fn, args in re.findall(r'(?<=[;{}])\s*([\w\s*]+?)\s*\b(mvsdf_\w+)\s*\(([^()]*)\)\s*;', ';' + text):
        ret = ' '.join(ret.replace('*', ' * ').split())
        if fn in protos:
            raise MvsdfError('%s is declared twice' % fn)
        args = [] if args.strip() in ('', 'void') else args.split(',')
        restype = None if ret == 'void' else C.c_char_p if ret == 'const char *' else _ctype(ret, fn, False)
        protos[fn] = (restype, [_ctype(a, fn, True) for a in args])
    unparsed = set(re.findall(r'\b(mvsdf_\w+)\s*\(', text)) ^ set(protos)                # a name followed by `(` that the pattern above did not take
    if unparsed:
        raise MvsdfError('cannot parse the declaration of %s' % ', '.join(sorted(unparsed)))
    return protos


def parse_constants(text):
    """{name: value} of every enumerator of a C header's anonymous enums.  A value is a decimal or hex literal or a shift of two; anything else is an error."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    consts = {}
    for body in re.findall(r'\benum\s*\{([^{}]*)\}\s*;', text):
        for item in filter(None, (i.strip() for i in body.split(','))):
            name, _, expr = (w.strip() for w in item.partition('='))
            m = re.fullmatch(r'(0[xX][0-9a-fA-F]+|\d+)(?:\s*<<\s*(0[xX][0-9a-fA-F]+|\d+))?', expr)
            if not m:
                raise MvsdfError('enumerator %s: %s' % (name, 'cannot evaluate "%s"' % expr if expr else 'no explicit value'))
            if name in consts:
                raise MvsdfError('enumerator %s is declared twice' % name)
            consts[name] = int(m.group(1), 0) << int(m.group(2) or '0', 0)
    return consts


class _Namespace:
    def __init__(self, d):
        self.__dict__.update(d)


try:
    with open(HEADER_PATH) as _f:
        _text = _f.read()
    PROTOTYPES = parse_header(_text)
    K = _Namespace(parse_constants(_text))                      # K.MVSDF_*: the result words, error bits and limits the header declares
except OSError as e:
    raise MvsdfError('the C header %s cannot be read (%s): the ctypes prototypes are derived from it, the package needs include/ beside it' % (HEADER_PATH, e)) from None
EXPORTS = list(PROTOTYPES)                                       # every symbol include/mvsdf_hip.h declares


def check(rc, what=''):
    if rc != 0:
        raise MvsdfError('%s failed (code %d): %s' % (what or 'mvsdf call', rc, lib().mvsdf_last_error().decode()))


def raise_for_bits(err, what, table):
    """raise for the first row (bit, exception class, message) of `table` whose bit is set in the error word; any other bit is a library error"""
    for bit, exc, message in table:
        if err & bit:
            raise exc('%s: %s' % (what, message))
    if err:
        raise MvsdfError('%s failed (error bits %d)' % (what, err))


def ptr(t):
    """device (or host) pointer of a contiguous torch tensor, or None."""
    if t is None:
        return None
    assert t.is_contiguous(), 'tensor must be contiguous'
    return C.c_void_p(t.data_ptr())


def stream_of(t):
    import torch
    if t.is_cuda:
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return C.c_void_p(0)


# what the scene-side modules (mesh, chamfer, cloud, fusion, raster, stereo, viewsel) pass to their calls: raw addresses, no contiguity check
def _vp(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _header(ws, n):
    """the int64 results a call leaves at the start of its workspace (reading them waits for the stream)"""
    import torch
    return [int(x) for x in ws[:8 * n].view(torch.int64).cpu()]


def f64_from_bits(bits):
    """the fp64 value a header word holds as its int64 bit pattern"""
    return struct.unpack('<d', struct.pack('<q', bits))[0]
