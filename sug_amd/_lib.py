"""ctypes binding of libsug_amd.so (the C ABI declared in include/sug_amd.h).

There is no CPU or eager fallback: if the library is missing or a tensor is not on
a HIP device, the calling op raises.
"""
import ctypes
import os
import re

# torch must be imported before libsug_amd.so is opened: both need libamdhip64.so.7 and the
# process must end up with ONE HIP runtime (torch's bundled copy), otherwise launches from this
# library see "no ROCm-capable device".
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libsug_amd.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'sug_amd.h')

_vp, _i32, _i64, _f32, _f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double

_SCALARS = {'int': _i32, 'int32_t': _i32, 'int64_t': _i64, 'uint64_t': ctypes.c_uint64, 'float': _f32, 'double': _f64}
_RESTYPES = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char*': ctypes.c_char_p}


def parse_header(text):
    """The C ABI from the header's text: ({name: (restype, [argtypes])} for every declaration, {SUG_NAME: int} for every
    object-like #define with an integer value).  Strict: whatever does not fit raises ValueError, nothing is skipped."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)         # comments hold ';', '(' and function names
    guard = re.search(r'^[ \t]*#[ \t]*ifndef[ \t]+(\w+)', text, flags=re.M)
    constants, code = {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith('#'):
            code.append(line)
            continue
        if line.rstrip().endswith('\\'):
            raise ValueError('sug_amd.h: a continued preprocessor line is not supported: %r' % line.strip())
        m = re.match(r'\s*#\s*define\s+(SUG_\w+)(\(?)(.*)', line)
        if not m or m.group(2):                                         # not a SUG_* define, or a function-like macro
            continue
        name, value = m.group(1), m.group(3).strip()
        if not value and guard and name == guard.group(1):              # the include guard
            continue
        if value.startswith('(') and value.endswith(')'):
            value = value[1:-1].strip()
        lit = re.fullmatch(r'(-?)\s*(0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)[uU]?', value)
        if not lit:
            raise ValueError('sug_amd.h: #define %s is not an integer literal: %r' % (name, line.strip()))
        constants[name] = int(lit.group(1) + lit.group(2), 0)
    code = re.sub(r'extern\s+"C"\s*\{(.*)\}', r'\1', '\n'.join(code), flags=re.S)
    functions = {}
    *decls, tail = code.split(';')
    if tail.strip():
        raise ValueError('sug_amd.h: text behind the last declaration: %r' % ' '.join(tail.split()))
    for decl in decls:
        decl = re.sub(r' ?\* ?', '* ', ' '.join(decl.split()))
        m =re.fullmatch(r'(const char\*|int64_t|int) (\w+) ?\((.*)\)', decl)
        if not m or not m.group(2).startswith('sug_') or m.group(2) in functions:
            raise ValueError('sug_amd.h: not a declaration of a new sug_* function returning int, int64_t or const char*: %r' % decl)
        args = []
        for param in ([] if m.group(3).strip() == 'void' else m.group(3).split(',')):
            words = param.split()
            if '[' in param or '(' in param:
                raise ValueError('sug_amd.h: array or function parameter %r in %r' % (param.strip(), decl))
            if '*' in param:
                args.append(_vp)
            elif len(words) == 2 and words[0] in _SCALARS and words[1].isidentifier():
                args.append(_SCALARS[words[0]])
            else:
                raise ValueError('sug_amd.h: parameter %r in %r is neither a pointer nor a known scalar' % (param.strip(), decl))
        functions[m.group(2)] = (_RESTYPES[m.group(1)], args)
    return functions, constants


def _header_text():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError('sug_amd: %s not found -- the ctypes binding is derived from it; keep include/ beside the '
                           'package, there is no fallback path' % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return f.read()


# Declaring an entry point in the header is its whole registration: DECLARATIONS holds every declaration as
# name -> (restype, argtypes), CONSTANTS every integer #define; SIGNATURES keeps the argtypes of the status-returning ones.
DECLARATIONS, CONSTANTS = parse_header(_header_text())
SIGNATURES = {name: args for name, (res, args) in DECLARATIONS.items() if res is ctypes.c_int and args}

STATS_BLOCKS = CONSTANTS['SUG_STATS_BLOCKS']

_lib = None


def lib():
    """Load (once) and return the library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'sug_amd: %s not found -- build it with `make -C sug_amd/csrc` or '
                '`python -c "import __graft_entry__ as g; g.build()"`; there is no fallback path'
                % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in DECLARATIONS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        if L.sug_abi_version() != CONSTANTS['SUG_ABI_VERSION']:
            raise RuntimeError('sug_amd: ABI version mismatch, rebuild libsug_amd.so')
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError('%s failed (%d): %s' % (what, rc, lib().sug_last_error().decode()))
