"""CPU: the C-ABI library loads and exports exactly what include/sug_amd.h declares."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NOT_IN_SIGNATURES = ('sug_last_error', 'sug_abi_version', 'sug_linear_dw_workspace', 'sug_adam_chunk', 'sug_adam_chain_chunk',
                     'sug_pointmlp_max_bwd_workspace', 'sug_ptran_colsum_workspace', 'sug_colsum_workspace',
                     'sug_chamfer_workspace', 'sug_scatter_rows_workspace')
CODES = {'p': ctypes.c_void_p, 'i': ctypes.c_int, 'l': ctypes.c_int64, 'u': ctypes.c_uint64, 'f': ctypes.c_float,
         'd': ctypes.c_double}
# Written by hand from the prototypes, one letter of CODES per parameter: the declarations that reach the parser's corners.
EXPECTED = {
    'sug_prepare_batch': (ctypes.c_int, 'piipiii' 'pppp' 'up' 'ff' 'ppppp'),       # uint64_t by value, const uint64_t*
    'sug_icp_fitness': (ctypes.c_int, 'plp' 'iii' 'didd' 'ppppp'),                 # doubles by value
    'sug_last_error': (ctypes.c_char_p, ''),                                      # const char* f(void)
    'sug_linear_dw_workspace': (ctypes.c_int64, 'lii'),                           # int64_t return
    'sug_adam_chunk': (ctypes.c_int, ''),                                         # int f(void)
    'sug_bn_replay_multi': (ctypes.c_int, 'i' 'ppp' 'p' 'pp' 'p'),                 # const void* const*, void* const*
    'sug_edgeconv_path': (ctypes.c_int, 'iiiii'),                                 # a query: ints only, no stream
}


def test_library_built_and_exports_header_symbols():
    from sug_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), 'build with make -C sug_amd/csrc'
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = sorted(_lib.DECLARATIONS)
    assert len(names) >= 177
    for n in names:
        assert hasattr(L, n), 'missing export %s' % n


def test_ctypes_table_matches_header():
    """Every declaration of the header is bound with its types; SIGNATURES holds the ones that return a status and take
    arguments."""
    from sug_amd import _lib
    declared = sorted(_lib.parse_header(open(os.path.join(ROOT, 'include', 'sug_amd.h')).read())[0])
    assert sorted(_lib.DECLARATIONS) == declared and set(NOT_IN_SIGNATURES) <= set(declared)
    assert sorted(_lib.SIGNATURES) == [n for n in declared if n not in NOT_IN_SIGNATURES]
    for n in _lib.SIGNATURES:
        assert _lib.SIGNATURES[n] is _lib.DECLARATIONS[n][1] and _lib.DECLARATIONS[n][0] is ctypes.c_int, n
    L = _lib.lib()
    for n, (res, args) in _lib.DECLARATIONS.items():
        assert getattr(L, n).restype is res and list(getattr(L, n).argtypes) == args, n


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_derived_binding_matches_hand_written_expectation(name):
    from sug_amd import _lib
    res, codes = EXPECTED[name]
    assert _lib.DECLARATIONS[name] == (res, [CODES[c] for c in codes])
    assert (name in _lib.SIGNATURES) == (res is ctypes.c_int and codes != '')


# ------------------------------------------------------------------------------------------ the parser, on header strings
def _parse(body):
    from sug_amd import _lib
    return _lib.parse_header('#ifndef SUG_AMD_H\n#define SUG_AMD_H\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n'
                             + body + '\n#ifdef __cplusplus\n}\n#endif\n#endif /* SUG_AMD_H */\n')


def test_parser_multi_line_declaration_and_comments():
    fns, consts = _parse('''
/* int sug_fake(int a); a comment with a ; and a ( and a declaration in it */
int sug_two_lines(const float* x, int64_t ldx,   // int sug_fake2(void);
                  int32_t n, uint64_t seed, const void* const* list,
                  float a, double b, uint8_t* arg, void* stream);
int64_t sug_ws(int64_t rows);
const char* sug_msg(void);
int sug_none(void);
''')
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert fns == {'sug_two_lines': (I, [P, L, I, ctypes.c_uint64, P, ctypes.c_float, ctypes.c_double, P, P]),
                   'sug_ws': (L, [L]), 'sug_msg': (ctypes.c_char_p, []), 'sug_none': (I, [])}
    assert consts == {}


@pytest.mark.parametrize('decl', ['int sug_f(size_t n);',                 # an unknown scalar type
                                  'int sug_f(float x[4]);',               # an array parameter
                                  'int sug_f(struct sug_args a);',        # a struct by value
                                  'int sug_f(sug_args_t a);',
                                  'int other_f(int n);',                  # a name outside the sug_ namespace
                                  'float sug_f(int n);',                  # a return type the binding does not know
                                  'int sug_f(int (*cb)(int));',           # a callback
                                  'int sug_f(int);',                      # an unnamed parameter
                                  'int sug_f(int n); int sug_f(int n);',  # declared twice
                                  'typedef struct { int a; } sug_args_t;',
                                  'int sug_f(int n)'])                    # no terminating semicolon
def test_parser_refuses_what_does_not_fit(decl):
    with pytest.raises(ValueError) as e:
        _parse('int sug_ok(int n);\n' + decl)
    assert 'sug_amd.h' in str(e.value) and decl.split(';')[0].split('(')[0].split()[-1] in str(e.value)     # quotes the declaration


def test_parser_constant_forms():
    _, consts = _parse('''
#define SUG_DEC 4096
#define SUG_HEX 0x20000000u
#define SUG_U 7u
#define SUG_NEG (-2)           /* a comment behind the value */
#define SUG_PAREN (12)
#define SUG_ZERO 0
#define SUG_WORDS(cap) (SUG_DEC + (cap))
#define NOT_OURS 1.5
''')
    assert consts == {'SUG_DEC': 4096, 'SUG_HEX': 0x20000000, 'SUG_U': 7, 'SUG_NEG': -2, 'SUG_PAREN': 12, 'SUG_ZERO': 0}
    for bad in ('#define SUG_X 1.5', '#define SUG_X (SUG_DEC + 1)', '#define SUG_X "s"', '#define SUG_X', '#define SUG_X 1 << 20',
                '#define SUG_X 010', '#define SUG_X \\\n 4'):
        with pytest.raises(ValueError, match='SUG_X'):
            _parse('#define SUG_DEC 4096\n' + bad)


def test_missing_header_names_the_path(monkeypatch):
    from sug_amd import _lib
    monkeypatch.setattr(_lib, 'HEADER_PATH', os.path.join(ROOT, 'include', 'no_such_header.h'))
    with pytest.raises(RuntimeError, match='no_such_header.h not found'):
        _lib._header_text()


def test_python_constants_are_the_headers():
    """The Python names that mirror a #define are read from the header (the literals below restate it on purpose)."""
    from sug_amd import _lib, ops, optim
    H = _lib.CONSTANTS
    assert H['SUG_ABI_VERSION'] == 8 and H['SUG_ERR_ARG'] == -1 and H['SUG_PREP_DRAW_NOISE'] == 0x20000000
    assert _lib.STATS_BLOCKS == H['SUG_STATS_BLOCKS'] == 1024
    assert (optim.CHAIN_SLOTS, optim.CHAIN_BUCKETS) == (2, 8)
    assert (ops.EVAL_MAX_ROWS, ops.EVAL_MAX_CLASSES, ops.EVAL_BATCH_COUNT, ops.EVAL_DATA_TOTAL, ops.EVAL_CORRECT_TOTAL,
            ops.EVAL_ERROR, ops.EVAL_LOSS_TOTAL, ops.EVAL_CLASS_ACC, ops.EVAL_CLASS_ROWS, ops.EVAL_CLASS_CORRECT,
            ops.EVAL_BATCH_ACC) == (4096, 64, 0, 1, 2, 3, 4, 8, 136, 200, 264)
    assert (ops.PREP_NORMALIZE, ops.PREP_ROTATE_Z, ops.PREP_JITTER, ops.PREP_SHUFFLE, ops.PREP_MAX_POINTS) == (1, 2, 4, 8, 4096)
    assert (ops.CE_MAX_ROWS, ops.CE_MAX_CLASSES, ops.MCD_MAX_ROWS, ops.MCD_MAX_CLASSES) == (1024, 64, 1024, 64)
    assert (ops.CLASS_MMD_MAX_ROWS, ops.CLASS_MMD_MAX_CLASSES, ops.CLASS_MMD_MAX_D) == (1024, 64, 1 << 20)
    assert (ops.ICP_MAX_POINTS, ops.KPCONV_MAX_CLOUD) == (1024, 4096)
    assert (ops.CE_PAIR_MAX_ROWS, ops.CE_PAIR_MAX_CLASSES) == (H['SUG_CE_PAIR_MAX_ROWS'], H['SUG_CE_PAIR_MAX_CLASSES']) == (512, 32)


# --------------------------------------------------------------------------- the limits of the header, one past each
def _host_buffer():
    """A real, writable host buffer: the calls below are refused before any launch, and would not read it either."""
    return ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)


def _refused(rc, limit):
    from sug_amd import _lib
    msg = _lib.lib().sug_last_error().decode()
    assert rc == -1 and re.search(r'\b%d\b' % limit, msg), (rc, msg)
    return msg


def test_mmd_select_limits_are_checked_on_the_host():
    from sug_amd import _lib
    L, H, p = _lib.lib(), _lib.CONSTANTS, _host_buffer()
    m, nc = H['SUG_CLASS_MMD_MAX_ROWS'], H['SUG_CLASS_MMD_MAX_CLASSES']
    assert 'sug_mmd_select: m=%d' % (m + 1) in _refused(L.sug_mmd_select(p, p, m + 1, 10, 0, p, p, p, p, p, None), m)
    assert 'num_class=%d' % (nc + 1) in _refused(L.sug_mmd_select(p, p, 8, nc + 1, 0, p, p, p, p, p, None), nc)
    d = H['SUG_CLASS_MMD_MAX_D']
    rc = L.sug_class_mmd_fwd(p, d + 1, p, d + 1, 8, d + 1, p, p, p, p, 5, p, None, p, p, None)
    assert 'sug_class_mmd_fwd' in _refused(rc, d)


def test_prepare_batch_limit_is_checked_on_the_host():
    from sug_amd import _lib
    L, p = _lib.lib(), _host_buffer()
    P = _lib.CONSTANTS['SUG_PREP_MAX_POINTS']
    rc = L.sug_prepare_batch(p, 4, P + 1, p, 2, P + 1, 1, None, None, None, None, 0, p, 0.01, 0.05, p, None, None, None, None)
    assert 'sug_prepare_batch: P=%d' % (P + 1) in _refused(rc, P)


def test_icp_fitness_limit_is_checked_on_the_host():
    from sug_amd import _lib
    L, p = _lib.lib(), _host_buffer()
    n = _lib.CONSTANTS['SUG_ICP_MAX_POINTS']
    for Ns, Nt in ((n + 1, 8), (8, n + 1)):
        rc = L.sug_icp_fitness(p, 0, p, 1, Ns, Nt, 0.15, 30, 1e-6, 1e-6, p, p, p, p, None)
        assert 'sug_icp_fitness: Ns=%d, Nt=%d' % (Ns, Nt) in _refused(rc, n)


def test_ce_pair_limits_are_checked_on_the_host():
    from sug_amd import _lib
    L, H, p = _lib.lib(), _lib.CONSTANTS, _host_buffer()
    rows, classes = H['SUG_CE_PAIR_MAX_ROWS'], H['SUG_CE_PAIR_MAX_CLASSES']
    for M, C in ((rows // 2 + 1, 10), (4, classes + 1)):
        msg = _refused(L.sug_ce_pair_fwd(p, p, C, p, M, C, 1.0, -100, p, p, None), rows)
        assert 'sug_ce_pair_fwd: M=%d rows, C=%d classes' % (M, C) in msg and re.search(r'\b%d\b' % classes, msg)
        assert L.sug_ce_pair_bwd(p, p, C, p, M, M, C, 1.0, -100, p, p, p, p, None) == -1
        assert b'sug_ce_pair_bwd' in L.sug_last_error()


def test_version_and_error_string():
    from sug_amd import _lib
    L = _lib.lib()
    assert L.sug_abi_version() == _lib.CONSTANTS['SUG_ABI_VERSION']
    # argument validation happens on the host before any launch: safe without a GPU
    rc = L.sug_knn(None, 3, 1, 8, 3, 4, None, None)
    assert rc == -1 and b'null' in L.sug_last_error()
    rc = L.sug_knn(ctypes.c_void_p(16), 3, 1, 8, 3, 40, ctypes.c_void_p(16), None)
    assert rc == -1 and b'k' in L.sug_last_error()


def test_interp3_cat_bwd_lists_supported_is_the_reverse_list_limit():
    """sug_interp3_cat_bwd_lists_supported says beforehand what sug_interp3_cat_bwd_lists would refuse (host-side checks,
    before any launch: safe without a GPU)."""
    from sug_amd import _lib
    L = _lib.lib()
    assert L.sug_interp3_cat_bwd_lists_supported(2, 12288, 8) == 1
    assert L.sug_interp3_cat_bwd_lists_supported(64, 1024, 64) == 1
    assert L.sug_interp3_cat_bwd_lists_supported(2, 13637, 8) == 1       # (2*8 + 32 + 3N) * 4 <= 160 KB
    assert L.sug_interp3_cat_bwd_lists_supported(2, 13638, 8) == 0
    assert L.sug_interp3_cat_bwd_lists_supported(2, 16384, 8) == 0
    assert L.sug_interp3_cat_bwd_lists_supported(0, 64, 8) == 0 and L.sug_interp3_cat_bwd_lists_supported(2, 64, 2) == 0
    p = ctypes.c_void_p(16)
    rc = L.sug_interp3_cat_bwd_lists(p, 12, 4, p, p, p, p, p, 2, 16384, 8, 8, p, p, p, p, p, None)
    assert rc == -1 and b'too many for the LDS-resident build' in L.sug_last_error()


def test_ops_refuse_cpu_tensors():
    import torch
    from sug_amd import ops
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.knn(torch.zeros(1, 8, 3), 4)
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.mix_rbf_mmd2_rows(torch.zeros(4, 8), 2)


def test_tuning_tables_are_well_formed():
    """sug_amd/tuning: the TunableOp table has validator lines + GEMM entries, and every weight-gradient
    shape routed to the library has a tuned TN entry with K = rows."""
    import csv
    import json
    from sug_amd import tuning
    rows = list(csv.reader(open(tuning.TABLE)))
    assert any(r[0] == 'Validator' and r[1] == 'GCN_ARCH_NAME' and r[2].startswith('gfx950') for r in rows)
    gemms = [r for r in rows if r[0].startswith('Gemm')]
    assert len(gemms) >= 20
    choice = json.load(open(tuning.DW_CHOICE))['library']
    keys = {r[1] for r in gemms}
    for R, M, N in choice:
        assert any(k.startswith('nt_%d_%d_%d_' % (N, M, R)) or k.startswith('tn_%d_%d_%d_' % (N, M, R)) or
                   ('_%d_' % R) in k for k in keys), (R, M, N)
