"""Host-only checks of tests/gemm_ref.py.  The Python restatement of csrc/gemm_route.h prints the routes tests/gemm_route_cli.cpp
prints, on the case table and on test_gemm_route_cpu.TABLE; the table reaches every instantiation of the written-out list; the
reference alone satisfies condition 2 (median bound <= rms / 128 for bf16, rms / 256 for fp32 outputs) at every shape; exact cases
are exact; and the bounds bite: a float64 emulation with the kernel's rounding points (bf16 operands, fp32-rounded sums of 64-wide
K steps, one rounding at the store) lies inside every bound, and each of eight faults is caught."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402
from test_gemm_route_cpu import TABLE, route_cli  # noqa: E402,F401  (the fixture compiles the CLI as that file's tests do)

F32, F64 = torch.float32, torch.float64
ID = lambda c: c.id
GEMM_CASES = [c for c in R.CASES if c.entry in ('gemm', 'dw')]


def test_route_restatement_equals_the_cli(route_cli):  # noqa: F811
    rows = [(name, call) for name, call, _ in TABLE] + [(f'case{i}', R.cli_line(c)) for i, c in enumerate(GEMM_CASES)]
    stdin = ''.join(f'{name} {call}\n' for name, call in rows)
    r = subprocess.run([route_cli], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split(' ', 1) for line in r.stdout.splitlines())
    wrong = []
    for name, call in rows:
        c, knobs, n_cu, det = R.parse_call(call)
        mine = R.cli_text(R.gemm_route(c, knobs, n_cu, det), c)
        if mine != got.get(name):
            wrong.append(f'{name}: {call}\n    python {mine}\n    cli    {got.get(name)}')
    assert not wrong, 'the restatement disagrees with gemm_route.h:\n  ' + '\n  '.join(wrong)
    recorded = {name: route for name, _, route in TABLE}
    assert all(got[name] == recorded[name] for name in recorded)


def test_case_lines_parse_back_to_the_case():
    for c in GEMM_CASES:
        call, knobs, n_cu, det = R.parse_call(R.cli_line(c))
        assert R.route(call, knobs, n_cu, det) == R.case_route(c), c.id


def test_route_table_is_complete():
    got, want = R.table_routes(), R.all_routes()
    assert got == want, (sorted(want - got), sorted(got - want))
    assert len(want) == 8 + 6 + 4 + 2 + 3 + 4 + 5 + 1 + 2
    # the cases reach the kernel their name says, through the per-call switches alone
    for c in R.CASES:
        r = R.case_route(c)
        fam = {'c': 'g256<', 'bk': 'g256<', 'g3': 'gemm3<', 'dw': 'g256dw<', 'g128': 'g128<a', 'skinny': 'skinny<', 'ws': 'g128<0,0,1>+reduce',
               'colsum': 'colsum_kernel'}
        key = next(k for k in ('colsum', 'skinny', 'g128', 'dw', 'g3', 'bk', 'ws', 'c') if c.name.startswith(k))
        assert fam[key] in r, (c.id, r)
        if c.name[0] == 'c' and c.name[1:].isdigit():
            assert f'epi={c.name[1:]}>' in r, (c.id, r)
        assert not set(c.env) - {'min_tiles', 'gemm3', 'ksplit', 'fold', 'dw_splits'}
    # reservations below 9 CUs are ignored by g256_cus: n_cu - 3 changes nothing, n_cu - 9 leaves 9 workgroups
    assert R.effective_cus(256, 253) == 256 and R.effective_cus(256, 247) == 9
    assert all(((c.M + 255) // 256) * ((c.N + 255) // 256) >= 12 for c in R.CASES if c.reserve)
    big = next(c for c in R.CASES if c.name == 'dw2g')
    assert (big.K + 512) * big.lda * 2 >= 2 ** 32 > (big.K + 511) * big.lda * 2
    call, knobs = R.call_of(big), R.knobs_of(big)
    assert R.cli_text(R.gemm_route(call, knobs, 256, True), call) == 'dw kc=42112 chunks=2 full=5/1/658/none tail=5/1/2/none'
    assert R.gemm_route(call, knobs, 256, False).chunk_error
    short = next(c for c in R.CASES if c.env.get('dw_splits'))
    r = R.gemm_route(R.call_of(short), R.knobs_of(short), 256, False)
    assert (short.K + 63) // 64 % r.full[2] != 0 and r.full[1] == 4


@pytest.mark.parametrize('c', R.CASES, ids=ID)
def test_conditions_on_the_reference_alone(c):
    for regime in R.REGIMES:
        if c.entry == 'colsum' and regime == 'address':
            continue
        d = R.inputs(c, regime)
        res = R.reference(c, d)
        for name, r in res.items():
            b = r.bound.expand_as(r.ref)
            assert bool(torch.isfinite(r.ref).all()) and bool(torch.isfinite(b).all()) and bool((b >= 0).all()), (regime, name)
            assert bool(((R.kernel_rounded(r) - r.ref).abs() <= b).all()), (regime, name)
            if regime == 'normal':
                assert R.condition_ii(r) <= R.ii_max(r), (name, R.condition_ii(r), r.k)
        if R.is_exact(c, regime):
            R.assert_exact_inputs(c, res)
            if c.drop:
                assert d.drop[3] == 2.0


# ------------------------------------------------------------------------------------------------- the bounds bite
def emulate_acc(fault=None):
    """float64 sums of bf16 products, rounded to fp32 after every 64-wide K step -> acc_of for gemm_ref.reference"""
    def acc_of(A, B):
        K = A.shape[1]
        Af = A.clone()
        if fault == 'kperm':                                   # A's k order permuted inside every 64-step (B's is not)
            for k0 in range(0, K, 64):
                w = min(64, K - k0)
                Af[:, k0:k0 + w] = A[:, k0:k0 + w].roll(w // 2 + 1, 1)
        last = (K - 1) // 64 * 64
        acc = torch.zeros(A.shape[0], B.shape[0], dtype=F64)
        for k0 in range(0, K, 64):
            if fault == 'ragged_skipped' and k0 == last and K % 64:
                continue
            acc = (acc + Af[:, k0:k0 + 64] @ B[:, k0:k0 + 64].t()).to(F32).to(F64)
        kd = K // 2
        if fault == 'dropped':
            acc = acc - A[:, kd:kd + 1] @ B[:, kd:kd + 1].t()
        if fault == 'twice':
            acc = acc + A[:, kd:kd + 1] @ B[:, kd:kd + 1].t()
        return acc, A.abs() @ B.abs().t()
    return acc_of


def emulate(c, d, fault=None):
    """the kernel's result on inputs d with ``fault`` built in, rounded once at the store"""
    d = R.NS(**vars(d))
    if fault == 'bias_shift':
        d.bias = d.bias.roll(1)
    if fault == 'alpha_after_bias':                            # alpha (acc + bias) = alpha acc + alpha bias
        d.bias = d.bias * d.alpha * R.norm_factor(d.asq)
    if fault == 'res_ldc_for_ldr':                             # residual[m][n] read at m ldc + n of its [M][ldr] storage
        st = torch.zeros(c.M * c.ldr + c.N, dtype=F64)
        st[:c.M * c.ldr].view(c.M, c.ldr)[:, :c.N] = d.res
        d.res = torch.as_strided(st, (c.M, c.N), (c.ldc, 1)).clone()
    if fault == 'drop_third':
        d.drop = (d.drop[0], d.drop[1] + 1, d.drop[2], d.drop[3])
    return R.kernel_rounded(R.reference(c, d, acc_of=emulate_acc(fault))['C'])


EMU = [R.case('emu128', 129, 136, 200, f32=1, bias=1, res=1, ldr=140, alpha=0.5, env=dict(min_tiles=R.BIG)),
       R.case('emu256', 257, 264, 128, bias=1, drop=2, alpha=0.5, env=dict(min_tiles=1)),
       R.case('emuskinny', 17, 72, 136, bias=1, res=1, ldr=80)]
FAULTS = ['dropped', 'twice', 'ragged_skipped', 'bias_shift', 'res_ldc_for_ldr', 'alpha_after_bias', 'drop_third', 'kperm']


def _applies(c, fault):
    return {'alpha_after_bias': c.alpha != 1, 'ragged_skipped': c.K % 64 != 0, 'res_ldc_for_ldr': bool(c.res) and c.ldr != c.ldc, 'drop_third': c.drop == 2}.get(fault, True)


@pytest.mark.parametrize('c', EMU, ids=ID)
def test_emulation_is_inside_and_faults_are_caught(c):
    assert (c.M, c.N, c.K) in {(t.M, t.N, t.K) for t in R.CASES}, 'emulation shapes come from the table'
    caught = {f: [] for f in FAULTS if _applies(c, f)}
    for regime in R.REGIMES:
        d = R.inputs(c, regime)
        r = R.reference(c, d)['C']
        got = emulate(c, d)
        if R.is_exact(c, regime):
            assert torch.equal(got, R.kernel_rounded(r)), regime
        units = ((got - r.ref).abs() / r.bound.clamp_min(1e-300)).max()
        print(f'UNITS emulation {c.id} {regime}: {float(units):.4f}')
        assert float(units) <= 1.0, (regime, float(units))
        for f in caught:
            bad = emulate(c, d, f)
            hit = (bad != R.kernel_rounded(r)) if R.is_exact(c, regime) else ((bad - r.ref).abs() > r.bound)
            if bool(hit.any()):
                caught[f].append(f'{regime} {float(hit.double().mean()):.2f}')
    print('CAUGHT', c.id, caught)
    for f, where in caught.items():
        assert where, f'{f} passes every regime'
        if f == 'kperm':
            assert any(w.startswith('address') for w in where), 'the address regime must catch a K permutation on one operand'
        if f in ('dropped', 'twice'):
            assert any(w.startswith('lattice') for w in where) and any(w.startswith('normal') for w in where), where


def test_every_fault_was_applied_somewhere():
    assert all(any(_applies(c, f) for c in EMU) for f in FAULTS)
