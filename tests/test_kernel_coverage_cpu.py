"""Every entry point bound in image2text_amd/lib.py::SIGNATURES has a direct kernel test: the ops.py wrapper(s) whose body names
it are called by at least one tests/test_*_gpu.py file (read as text).  What has none is listed in NO_DIRECT_TEST, with the reason;
a new entry point added without a kernel test fails here."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry point -> why no test calls a wrapper of it directly.  Only: graph capture and communicator calls and ABI / error / workspace /
# mode queries.
NO_DIRECT_TEST = {
    'i2t_abi_version': 'query: checked on every load (lib.load) and in tests/test_abi.py',
    'i2t_last_error': 'query: read through lib.last_error by every refusal test',
    'i2t_workspace_bytes': 'query: host arithmetic, no kernel',
    'i2t_deterministic': 'mode query: no kernel',
    'i2t_gemm_reserved_cus': 'mode query: no kernel',
    'i2t_moe_gate_bwd_blocks': 'workspace query of i2t_moe_gate_bwd: host arithmetic, no kernel',
    'i2t_graph_capture_begin': 'graph capture: runs under the decode-step and beam-search tests, no kernel of its own',
    'i2t_graph_capture_end': 'graph capture',
    'i2t_graph_launch': 'graph capture',
    'i2t_graph_destroy': 'graph capture',
    'i2t_comm_available': 'communicator: tests/test_dp_gpu.py runs it in child processes',
    'i2t_comm_unique_id': 'communicator',
    'i2t_comm_init': 'communicator',
    'i2t_comm_allreduce': 'communicator',
    'i2t_comm_destroy': 'communicator',
}
ALLOWED_PREFIXES = ('i2t_graph_', 'i2t_comm_')
ALLOWED_QUERIES = {'i2t_abi_version', 'i2t_last_error', 'i2t_workspace_bytes', 'i2t_deterministic', 'i2t_gemm_reserved_cus',
                   'i2t_moe_gate_bwd_blocks'}
VARIANT = re.compile(r'_(ex|eps|drop)$')


def _signature_names():
    """the keys of lib.py::SIGNATURES, read from the source (no torch import, no library load)"""
    tree = ast.parse(open(os.path.join(ROOT, 'image2text_amd', 'lib.py')).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, 'id', None) == 'SIGNATURES' for t in node.targets):
            return [k.value for k in node.value.keys]
    raise AssertionError('lib.py has no SIGNATURES table')


def _ops_functions():
    """{function name: source} of the top-level functions of ops.py"""
    src = open(os.path.join(ROOT, 'image2text_amd', 'ops.py')).read()
    return {n.name: ast.get_source_segment(src, n) for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}


def _public_callers(name, funcs, seen=()):
    """a private helper counts through the public wrappers that dispatch to it"""
    if not name.startswith('_'):
        return {name}
    out = set()
    for other, body in funcs.items():
        if other != name and other not in seen and re.search(rf'\b{re.escape(name)}\(', body):
            out |= _public_callers(other, funcs, seen + (name,))
    return out


def wrappers_of(entry, funcs, follow=True):
    out = set()
    for fn, body in funcs.items():
        if re.search(rf'\.{re.escape(entry)}\(', body):
            out |= _public_callers(fn, funcs)
    if not out and follow:                               # nothing names it: an _ex / _eps / _drop variant counts through the wrapper of
        base = VARIANT.sub('', entry)                    # its base, and a base that ops.py reaches only in its extended form through that
        for other in {base} | {f'{base}_{v}' for v in ('ex', 'eps', 'drop')}:
            if other != entry:
                out |= wrappers_of(other, funcs, follow=False)
    return out


def test_every_entry_point_has_a_direct_kernel_test():
    funcs = _ops_functions()
    gpu_tests = {p: open(p).read() for p in glob.glob(os.path.join(ROOT, 'tests', 'test_*_gpu.py'))}
    assert gpu_tests
    missing = []
    for entry in _signature_names():
        if entry in NO_DIRECT_TEST:
            continue
        ws = wrappers_of(entry, funcs)
        if not ws:
            missing.append(f'{entry}: no ops.py wrapper names it')
            continue
        for w in sorted(ws):
            if not any(re.search(rf'\bops\.{w}\(', text) for text in gpu_tests.values()):
                missing.append(f'{entry}: ops.{w} is called by no tests/test_*_gpu.py')
    assert not missing, 'entry points without a direct kernel test (add one, or a reasoned row in NO_DIRECT_TEST):\n  ' + '\n  '.join(missing)


def test_the_exemption_table_stays_narrow():
    names = set(_signature_names())
    for entry, reason in NO_DIRECT_TEST.items():
        assert entry in names, f'{entry} is not an entry point any more: drop its row'
        assert reason.strip(), entry
        assert entry.startswith(ALLOWED_PREFIXES) or entry in ALLOWED_QUERIES, f'{entry}: only capture / communicator calls and queries may go untested'
