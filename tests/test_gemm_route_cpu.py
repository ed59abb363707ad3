"""Which kernel an i2t_gemm_bf16 call reaches (image2text_amd/csrc/gemm_route.h), checked on the CPU: tests/gemm_route_cli.cpp is compiled
with the host C++ compiler (no HIP), fed the calls of TABLE and must print the routes of TABLE.

The expected routes were recorded from the launch code as it stood BEFORE the rule moved into gemm_route.h (its launches replaced by a
recorder of kernel, template arguments, grid, K slices and column-sum launches), not read off gemm_route.h: a row that fails says the
routing changed.  n_cu is 256 unless a row says otherwise.

Row = (name, call, route).  call: M N K, ak / bk = A / B k-major, f32 acc act drop as in i2t_gemm_bf16, bias auxi auxo res cso as = operand
present (cso: colsum_out, as: alpha_sumsq), resc = residual is C, c16 = C 16-byte aligned, alpha1 = alpha is 1, det = deterministic mode;
knobs: no_g256 (I2T_GEMM=v1), min_tiles, gemm3, narrow, ksplit, fold, dw_splits, gn, stagger, g256_dbg, g3_dbg, fp8_g256, log.
route: skinny mt ksplit | g128 splits | g256 cls | gemm3 cls overlap, each with colsum = none | before (a colsum_kernel launch first);
dw kc chunks full[ tail][ error] with a plan cls/splits/K-tiles per slice/colsum per chunk length (folded: inside the class-13 kernel;
error: the chunk after `chunks` has no large-tile form and the call fails there)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = [
    ('skinny_decode_m17', 'M=17 N=72 K=136',
     'skinny mt=2 ksplit=1 colsum=none'),
    ('skinny_m64_bias', 'M=64 N=768 K=768 bias=1',
     'skinny mt=4 ksplit=1 colsum=none'),
    ('m65_not_skinny', 'M=65 N=768 K=768 bias=1',
     'g128 splits=1 colsum=none'),
    ('skinny_gelu_m1', 'M=1 N=3072 K=768 bias=1 act=1',
     'skinny mt=1 ksplit=1 colsum=none'),
    ('m16_dgelu_not_skinny', 'M=16 N=768 K=3072 act=2 auxi=1',
     'g128 splits=1 colsum=none'),
    ('skinny_inplace_residual', 'M=16 N=768 K=3072 f32=1 res=1 resc=1',
     'skinny mt=1 ksplit=1 colsum=none'),
    ('skinny_inplace_residual_ksplit', 'M=16 N=768 K=3072 f32=1 res=1 resc=1 ksplit=1',
     'skinny mt=1 ksplit=8 colsum=none'),
    ('skinny_ksplit_needs_inplace', 'M=16 N=768 K=3072 f32=1 res=1 ksplit=1',
     'skinny mt=1 ksplit=1 colsum=none'),
    ('fwd_class1_bias', 'M=10240 N=1024 K=768 bias=1',
     'g256 cls=1 colsum=none'),
    ('fwd_class2_gelu', 'M=10240 N=1024 K=768 bias=1 act=1 auxo=1',
     'g256 cls=2 colsum=none'),
    ('fwd_class10_gelu_dout', 'M=10240 N=1024 K=768 bias=1 act=5 auxo=1',
     'g256 cls=10 colsum=none'),
    ('fwd_class3_f32_residual', 'M=10240 N=1024 K=768 bias=1 f32=1 res=1',
     'g256 cls=3 colsum=none'),
    ('fwd_class5_f32_plain', 'M=10240 N=1024 K=768 f32=1',
     'g256 cls=5 colsum=none'),
    ('fwd_class7_ragged_n', 'M=10240 N=1022 K=768 ldc=1024',
     'g256 cls=7 colsum=none'),
    ('fwd_class0_ldc_odd', 'M=10240 N=1022 K=768 ldc=1022',
     'g256 cls=0 colsum=none'),
    ('dx_class4_dgelu', 'M=10240 N=1024 K=768 bk=1 act=2 auxi=1',
     'g256 cls=4 colsum=none'),
    ('dx_class11_mul_aux', 'M=10240 N=1024 K=768 bk=1 act=6 auxi=1',
     'g256 cls=11 colsum=none'),
    ('dgelu_rowmajor_b_generic', 'M=10240 N=1024 K=768 act=2 auxi=1',
     'g256 cls=0 colsum=none'),
    ('gelu_kmajor_b_generic', 'M=10240 N=1024 K=768 bk=1 bias=1 act=1 auxo=1',
     'g256 cls=0 colsum=none'),
    ('k200_rowmajor_b_128', 'M=10240 N=1024 K=200',
     'g128 splits=1 colsum=none'),
    ('k200_kmajor_b_256', 'M=10240 N=1024 K=200 bk=1',
     'g256 cls=1 colsum=none'),
    ('k192_rowmajor_b_128', 'M=10240 N=1024 K=192',
     'g128 splits=1 colsum=none'),
    ('tiles39_128', 'M=9984 N=256 K=512',
     'g128 splits=1 colsum=none'),
    ('tiles40_256', 'M=10240 N=256 K=512',
     'g256 cls=1 colsum=none'),
    ('tiles40_min_tiles41', 'M=10240 N=256 K=512 min_tiles=41',
     'g128 splits=1 colsum=none'),
    ('min_tiles1_small', 'M=257 N=264 K=128 min_tiles=1',
     'g256 cls=1 colsum=none'),
    ('lora_n128', 'M=20480 N=128 K=4096',
     'g128 splits=1 colsum=none'),
    ('lora_n128_narrow', 'M=20480 N=128 K=4096 narrow=1',
     'g256 cls=1 colsum=none'),
    ('n129', 'M=20480 N=129 K=4096 ldc=132',
     'g256 cls=7 colsum=none'),
    ('no_g256', 'M=10240 N=1024 K=768 bias=1 no_g256=1',
     'g128 splits=1 colsum=none'),
    ('bench_fwd_m798720', 'M=798720 N=1536 K=512 bias=1 drop=2',
     'g256 cls=1 colsum=none'),
    ('bench_fwd_m798720_gemm3', 'M=798720 N=1536 K=512 bias=1 gemm3=2',
     'gemm3 cls=1 overlap=1 colsum=none'),
    ('gemm3_mode1', 'M=600 N=264 K=512 min_tiles=1 gemm3=1',
     'gemm3 cls=1 overlap=0 colsum=none'),
    ('gemm3_mode2_gelu', 'M=600 N=264 K=512 min_tiles=1 gemm3=2 bias=1 act=1 auxo=1',
     'gemm3 cls=2 overlap=1 colsum=none'),
    ('gemm3_mode0', 'M=600 N=264 K=512 min_tiles=1 gemm3=0',
     'g256 cls=1 colsum=none'),
    ('gemm3_c_misaligned', 'M=600 N=264 K=512 min_tiles=1 gemm3=1 c16=0',
     'g256 cls=1 colsum=none'),
    ('gemm3_alpha', 'M=600 N=264 K=512 min_tiles=1 gemm3=1 alpha1=0',
     'g256 cls=1 colsum=none'),
    ('gemm3_k256_too_short', 'M=600 N=264 K=256 min_tiles=1 gemm3=1',
     'g256 cls=1 colsum=none'),
    ('knobs_that_do_not_route', 'M=10240 N=1024 K=768 bias=1 gn=16 stagger=3 stagger_groups=4 g256_dbg=2 g3_dbg=1 fp8_g256=0 log=1',
     'g256 cls=1 colsum=none'),
    ('splitk_dw_small', 'M=128 N=136 K=4096 ak=1 bk=1 f32=1 acc=1',
     'g128 splits=16 colsum=none'),
    ('splitk_dw_small_det', 'M=128 N=136 K=4096 ak=1 bk=1 f32=1 acc=1 det=1',
     'g128 splits=1 colsum=none'),
    ('dw_lm_head_tied', 'M=50264 N=768 K=74000 ak=1 bk=1 f32=1 acc=1',
     'dw kc=42112 chunks=2 full=5/1/658/none tail=5/1/500/none'),
    ('dw_qwen2_down_proj', 'M=1536 N=8960 K=8192 ak=1 bk=1 f32=1 acc=1',
     'dw kc=8192 chunks=1 full=5/1/128/none'),
    ('dw_split', 'M=256 N=264 K=8192 ak=1 bk=1 f32=1 acc=1',
     'dw kc=8192 chunks=1 full=6/16/8/none'),
    ('dw_split_k1024', 'M=256 N=264 K=1024 ak=1 bk=1 f32=1 acc=1',
     'dw kc=1024 chunks=1 full=6/2/8/none'),
    ('dw_split_colsum_folded', 'M=256 N=264 K=8192 ak=1 bk=1 f32=1 acc=1 cso=1 as=1',
     'dw kc=8192 chunks=1 full=13/16/8/folded'),
    ('dw_split_colsum_unfolded', 'M=256 N=264 K=8192 ak=1 bk=1 f32=1 acc=1 cso=1 fold=0',
     'dw kc=8192 chunks=1 full=6/16/8/before'),
    ('dw_det_one_slice_colsum', 'M=256 N=264 K=8192 ak=1 bk=1 f32=1 acc=1 cso=1 det=1',
     'dw kc=8192 chunks=1 full=5/1/128/before'),
    ('dw_splits_knob', 'M=256 N=264 K=8192 ak=1 bk=1 f32=1 acc=1 dw_splits=4',
     'dw kc=8192 chunks=1 full=6/4/32/none'),
    ('dw_no_g256', 'M=256 N=264 K=8192 ak=1 bk=1 f32=1 acc=1 no_g256=1',
     'g128 splits=32 colsum=none'),
    ('dw_m255_128', 'M=255 N=264 K=8192 ak=1 bk=1 f32=1 acc=1 cso=1',
     'g128 splits=32 colsum=before'),
    ('dw_tiles128_split', 'M=2048 N=4096 K=4096 ak=1 bk=1 f32=1 acc=1',
     'dw kc=4096 chunks=1 full=6/2/32/none'),
    ('dw_tiles129_one_slice', 'M=768 N=11008 K=4096 ak=1 bk=1 f32=1 acc=1',
     'dw kc=4096 chunks=1 full=5/1/64/none'),
    ('dw_tiles128_cu248_one_slice', 'M=2048 N=4096 K=4096 ak=1 bk=1 f32=1 acc=1 n_cu=248',
     'dw kc=4096 chunks=1 full=5/1/64/none'),
    ('dw_first_chunk_falls_through', 'M=256 N=264 K=512 ak=1 bk=1 f32=1 acc=1 cso=1',
     'g128 splits=2 colsum=before'),
    ('dw_later_chunk_error', 'M=512 N=768 K=42312 lda=50264 ak=1 bk=1 f32=1 acc=1',
     'dw kc=42112 chunks=1 full=6/42/16/none tail=0/0/0/none error'),
    ('dw_chunked_split', 'M=512 N=768 K=74000 lda=50264 ak=1 bk=1 f32=1 acc=1 cso=1',
     'dw kc=42112 chunks=2 full=13/42/16/folded tail=13/42/12/folded'),
]


@pytest.fixture(scope='module')
def route_cli(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler found (set CXX)'
    exe = str(tmp_path_factory.mktemp('gemm_route') / 'gemm_route_cli')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', os.path.join(ROOT, 'tests', 'gemm_route_cli.cpp'), '-o', exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_routes_match_the_recorded_table(route_cli):
    stdin = ''.join(f'{name} {call}\n' for name, call, _ in TABLE)
    r = subprocess.run([route_cli], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split(' ', 1) for line in r.stdout.splitlines())
    wrong = [f'{name}: {call}\n    expected {route}\n    got      {got.get(name)}' for name, call, route in TABLE if got.get(name) != route]
    assert not wrong, 'routes changed:\n  ' + '\n  '.join(wrong)


def test_the_table_covers_every_route_class_and_knob():
    names = [name for name, _, _ in TABLE]
    assert len(set(names)) == len(names)
    routes = ' '.join(route for _, _, route in TABLE)
    for kind in ('skinny', 'g128 splits=1 ', 'g128 splits=16', 'g256', 'gemm3', 'dw', 'error', 'tail=', 'folded', 'before'):
        assert kind in routes, kind
    for cls in (0, 1, 2, 3, 4, 5, 7, 10, 11):
        assert f'g256 cls={cls} ' in routes, cls
    for cls in (5, 6, 13):
        assert f'full={cls}/' in routes, cls
    calls = ' '.join(call for _, call, _ in TABLE)
    for knob in ('no_g256', 'min_tiles', 'gemm3', 'narrow', 'ksplit', 'fold', 'dw_splits', 'gn', 'stagger', 'g256_dbg', 'g3_dbg', 'fp8_g256', 'log', 'det', 'n_cu'):
        assert f' {knob}=' in calls, knob
