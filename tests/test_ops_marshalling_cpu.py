"""The marshalling layer of image2text_amd/ops.py without a GPU: the pure operand check, the checked callers of every kernel entry
point against a recording stand-in for the library (the real one is never loaded), and ops.py read with ``ast`` -- nothing but the
checked caller turns a tensor into an address, and only the entry points listed in DIRECT are called on the library itself."""
import ast
import os
import types

import pytest
import torch

from image2text_amd import lib as i2tlib
from image2text_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry point -> why ops.py (or its caller elsewhere) calls it on the library directly, not through the checked caller
DIRECT = {
    'i2t_set_deterministic': 'no stream, no pointer: one int',
    'i2t_deterministic': 'no stream: a query without arguments',
    'i2t_gemm_reserve_cus': 'no stream, no pointer: one int',
    'i2t_gemm_reserved_cus': 'no stream: a query without arguments',
    'i2t_moe_gate_bwd_blocks': 'no stream: host arithmetic on one int',
    'i2t_abi_version': 'no stream: a query without arguments (lib.load)',
    'i2t_last_error': 'no stream: fills a host buffer (lib.last_error)',
    'i2t_workspace_bytes': 'no stream: host arithmetic, a host string in and a host long out',
    'i2t_graph_capture_begin': 'takes the stream being captured, no operand',
    'i2t_graph_capture_end': 'returns a graph handle through a host void**',
    'i2t_graph_launch': 'takes a graph handle, then the stream',
    'i2t_graph_destroy': 'takes a graph handle',
    'i2t_comm_available': 'no stream: a query without arguments',
    'i2t_comm_unique_id': 'fills a host buffer',
    'i2t_comm_init': 'host buffer in, a communicator handle out through a host void**',
    'i2t_comm_allreduce': 'takes a communicator handle first and a stream of its own (training/dp.py)',
    'i2t_comm_destroy': 'takes a communicator handle',
}
CHECKED = [name for name in i2tlib.SIGNATURES if name not in DIRECT]
TYPED = (i2tlib.PF, i2tlib.PI, i2tlib.PL, i2tlib.PN, i2tlib.PU)
DTYPES = (torch.float32, torch.int32, torch.int64, torch.bfloat16, torch.uint8, torch.float16, torch.float64, torch.int16, torch.bool)


class Recorder:
    """stands in for the loaded library: every i2t_* attribute records its arguments and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('i2t_'):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


def is_pointer(kind):
    return isinstance(kind, type) and issubclass(kind, i2tlib.P)


def test_the_direct_list_and_the_table_agree():
    assert set(DIRECT) <= set(i2tlib.SIGNATURES) and len(CHECKED) >= 100
    for name in CHECKED:
        row = i2tlib.SIGNATURES[name]
        assert row and row[0] is i2tlib.P, f'{name}: a checked entry point takes the stream first'
        assert any(is_pointer(k) for k in row[1:]), f'{name}: no operand after the stream'
    assert set(i2tlib.POINTER_DTYPE) == {i2tlib.P, *TYPED} and i2tlib.POINTER_DTYPE[i2tlib.P] is None
    assert [i2tlib.POINTER_DTYPE[k] for k in TYPED] == [torch.float32, torch.int32, torch.int64, torch.int64, torch.int32]


@pytest.mark.parametrize('kind', TYPED, ids=lambda k: k.__name__)
def test_a_typed_kind_takes_its_own_dtype_on_the_device_only(kind):
    own = i2tlib.POINTER_DTYPE[kind]
    assert ops.operand_error(kind, True, own) is None
    for dtype in DTYPES:
        if dtype != own:
            why = ops.operand_error(kind, True, dtype)
            assert why is not None and str(own) in why and str(dtype) in why
        assert 'no CPU path' in ops.operand_error(kind, False, dtype)


def test_a_void_pointer_refuses_only_the_device():
    for dtype in DTYPES:
        assert ops.operand_error(i2tlib.P, True, dtype) is None
        assert 'no CPU path' in ops.operand_error(i2tlib.P, False, dtype)


def host_arguments(name):
    """one argument per position after the stream: a one-element CPU tensor of the right dtype behind a pointer, 0 for a scalar"""
    return [torch.zeros(1, dtype=i2tlib.POINTER_DTYPE[k] or torch.bfloat16) if is_pointer(k) else 0 for k in i2tlib.SIGNATURES[name][1:]]


@pytest.mark.parametrize('name', CHECKED)
def test_no_kernel_entry_point_is_reached_with_a_host_address(name):
    rec = Recorder()
    k = ops._Kernels(lambda: rec)
    with pytest.raises(i2tlib.I2TError, match='no CPU path'):
        getattr(k, name)(*host_arguments(name))
    assert rec.calls == []
    n_ptr = sum(is_pointer(kind) for kind in i2tlib.SIGNATURES[name][1:])
    for skip in range(n_ptr):                                   # ... nor with one host operand among absent ones
        args, seen = host_arguments(name), -1
        for i, kind in enumerate(i2tlib.SIGNATURES[name][1:]):
            if is_pointer(kind):
                seen += 1
                if seen != skip:
                    args[i] = None
        with pytest.raises(i2tlib.I2TError, match='no CPU path'):
            getattr(k, name)(*args)
    assert rec.calls == []


class OnDevice:
    """what the checked caller reads of a device tensor"""
    is_cuda = True

    def __init__(self, dtype, address):
        self.dtype, self.address = dtype, address

    def data_ptr(self):
        return self.address


def test_a_checked_call_passes_stream_addresses_and_scalars(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda: types.SimpleNamespace(cuda_stream=77))
    rec = Recorder()
    k = ops._Kernels(lambda: rec)
    flag, a, out = OnDevice(torch.int32, 1000), OnDevice(torch.float32, 2000), OnDevice(torch.float32, 4000)
    assert i2tlib.SIGNATURES['i2t_select_rows'] == [i2tlib.P, i2tlib.PI, i2tlib.PF, i2tlib.PF, i2tlib.PF, i2tlib.L]
    k.i2t_select_rows(flag, a, None, out, 4)
    assert rec.calls == [('i2t_select_rows', (77, 1000, 2000, None, 4000, 4))]
    with pytest.raises(i2tlib.I2TError) as e:
        k.i2t_select_rows(OnDevice(torch.int64, 1000), a, a, out, 4)
    assert all(s in str(e.value) for s in ('i2t_select_rows', 'argument 0', 'torch.int32', 'torch.int64'))
    with pytest.raises(i2tlib.I2TError, match='i2t_select_rows: argument 2 wants a tensor or None, got int'):
        k.i2t_select_rows(flag, a, 3000, out, 4)
    bf16 = OnDevice(torch.bfloat16, 8)                          # void*: any dtype
    k.i2t_swiglu_fwd(bf16, 16, OnDevice(torch.uint8, 9), 2, 8)
    assert len(rec.calls) == 2 and rec.calls[1] == ('i2t_swiglu_fwd', (77, 8, 16, 9, 2, 8))


def _ops_tree():
    return ast.parse(open(os.path.join(ROOT, 'image2text_amd', 'ops.py')).read())


def test_ops_has_no_marshalling_but_the_checked_caller():
    tree = _ops_tree()
    names = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)} | {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} \
        | {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    assert not names & {'_p', '_need_cuda'}
    allowed = [n for n in tree.body if getattr(n, 'name', None) in ('_Kernels', '_lo_of')]
    assert len(allowed) == 2
    inside = {id(n) for top in allowed for n in ast.walk(top)}
    stray = [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr == 'data_ptr' and id(n) not in inside]
    assert not stray, f'ops.py takes an address outside the checked caller at lines {stray}'


def test_only_the_direct_entry_points_are_called_on_the_library():
    direct, checked = set(), set()
    for n in ast.walk(_ops_tree()):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr.startswith('i2t_'):
            recv = n.func.value
            if isinstance(recv, ast.Name) and recv.id == '_k':
                checked.add(n.func.attr)
            else:
                assert isinstance(recv, ast.Call) and getattr(recv.func, 'id', None) == '_lib', f'line {n.lineno}: {n.func.attr} on neither _k nor _lib()'
                direct.add(n.func.attr)
    assert direct <= set(DIRECT), direct - set(DIRECT)
    assert checked <= set(CHECKED), checked - set(CHECKED)
    assert len(checked) >= 100
