"""ctypes binding of libmvsdf_hip.so (C ABI: include/mvsdf_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, we raise.
"""
import ctypes as C
import os
import re
import struct

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get('MVSDF_LIB') or os.path.join(_HERE, 'libmvsdf_hip.so')   # MVSDF_LIB: dev override (ablation builds)
_lib = None


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


_COMMENTS = re.compile(r'/\*.*?\*/|//[^\n]*', re.S)


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
    text = _COMMENTS.sub(' ', text)
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


_LITERAL = r'(0[xX][0-9a-fA-F]+|\d+)(?:[ \t]*<<[ \t]*(0[xX][0-9a-fA-F]+|\d+))?'


def parse_constants(text):
    """{name: value} of every enumerator of a C header's anonymous enums, then of every `#define MVSDF_NAME <literal>`.  A value is a decimal or hex
    literal or a shift of two; in an enumerator anything else is an error, any other macro (the include guard, a function-like one) is left alone."""
    text = _COMMENTS.sub(' ', text)
    items = []
    for body in re.findall(r'\benum\s*\{([^{}]*)\}\s*;', text):
        for item in filter(None, (i.strip() for i in body.split(','))):
            name, _, expr = (w.strip() for w in item.partition('='))
            m = re.fullmatch(_LITERAL, expr)
            if not m:
                raise MvsdfError('enumerator %s: %s' % (name, 'cannot evaluate "%s"' % expr if expr else 'no explicit value'))
            items.append((name,) + m.groups())
    items += re.findall(r'^[ \t]*#[ \t]*define[ \t]+(MVSDF_\w+)[ \t]+%s[ \t]*$' % _LITERAL, text, flags=re.M)
    consts = {}
    for name, value, shift in items:
        if name in consts:
            raise MvsdfError('%s is declared twice' % name)
        consts[name] = int(value, 0) << int(shift or '0', 0)
    return consts


def parse_structs(text, consts=None):
    """{name: ctypes.Structure subclass} of every anonymous `typedef struct { ... } MvsdfName;` of a C header, in its order; `cls._fields_` is the
    ordered (field, ctype) list.  A member is `type a, b[N];`: a _SCALARS spelling or a struct declared earlier by value, c_void_p for anything with
    a `*`, N a decimal literal or one of `consts` (default: the header's own).  Anything else is an error that names the struct and the member."""
    text = _COMMENTS.sub(' ', text)
    consts = parse_constants(text) if consts is None else consts
    structs = {}
    pieces = re.split(r'typedef\s+struct\s*\{([^{}]*(?:\{[^{}]*\}[^{}]*)*)\}\s*(\w+)\s*;', text)     # [outside, body, name, outside, ...]
    for body, name in zip(pieces[1::3], pieces[2::3]):
        fields = []
        for decl in filter(None, (' '.join(d.split()) for d in re.sub(r'\{[^{}]*\}', '{}', body).split(';'))):
            def refuse(why):
                raise MvsdfError('%s, member "%s": %s' % (name, decl, why))
            m = re.fullmatch(r'([\w *]*[ *])(\w+ ?(?:\[[^\[\]]*\])?(?: ?, ?\w+ ?(?:\[[^\[\]]*\])?)*)', decl)
            if not m:
                refuse('not of the form `type a, b[N]` (no bit-field, union, nested struct, function pointer or second array dimension)')
            spelling = ' '.join(w for w in m.group(1).split() if w != 'const')
            if '*' in spelling and ',' in decl:
                refuse('a pointer declaration with more than one declarator')
            ctype = C.c_void_p if '*' in spelling else _SCALARS.get(spelling) or structs.get(spelling)
            if ctype is None:
                refuse('no ctypes mapping for the C type "%s" (a struct is declared before its use)' % spelling)
            for field, dim in re.findall(r'(\w+) ?(\[[^\[\]]*\])?', m.group(2)):
                n = dim[1:-1].strip()
                n = int(n) if n.isdecimal() else consts.get(n)
                if dim and not n:
                    refuse('cannot evaluate the array length %s' % dim)
                fields.append((field, ctype * n if dim else ctype))
        structs[name] = type(name, (C.Structure,), {'_fields_': fields})
    unparsed = re.search(r'\b(?:struct|union)\b.{0,60}', ' '.join(pieces[0::3]), flags=re.S)      # a keyword outside the blocks the pattern above took
    if unparsed:
        raise MvsdfError('cannot parse the declaration at "%s"' % ' '.join(unparsed.group(0).split()))
    return structs


class _Namespace:
    def __init__(self, d):
        self.__dict__.update(d)


try:
    with open(HEADER_PATH) as _f:
        _text = _COMMENTS.sub(' ', _f.read())                   # once for the three parsers
    PROTOTYPES = parse_header(_text)
    K = _Namespace(parse_constants(_text))                      # K.MVSDF_*: the result words, error bits and limits the header declares
    STRUCTS = parse_structs(_text, vars(K))                     # the header's structs as ctypes.Structure classes, in its order
except OSError as e:
    raise MvsdfError('the C header %s cannot be read (%s): the ctypes prototypes and structs are derived from it, the package needs include/ beside it' % (HEADER_PATH, e)) from None
EXPORTS = list(PROTOTYPES)                                       # every symbol include/mvsdf_hip.h declares
NetDesc, TraceParams, MAX_LAYERS = STRUCTS['MvsdfNetDesc'], STRUCTS['MvsdfTraceParams'], K.MVSDF_MAX_LAYERS


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
