"""Which kernels an attention call reaches (image2text_amd/csrc/attention_route.h), checked on the CPU: tests/attention_route_cli.cpp is
compiled with the host C++ compiler (no HIP), fed calls and must print their routes.  Three checks:

1. TABLE.  The expected routes were recorded from the host code of csrc/attention.hip and csrc/attention_g.hip as it stood BEFORE the
   rule moved into attention_route.h (that code copied, the environment variables set as strings, every launch replaced by a recorder
   of kernel name, template arguments, grid and block), not read off attention_route.h: a row that fails says the routing changed.
   The same recorder agreed with attention_route.h on the whole grid Tq, Tk in [1, 320] x causal x packed x dropout x out-drop x
   out_drop_q_seq in {0, Tq, 197, 320} under all 405 combinations of the five variables (unset and every value the code tells apart)
   before the table was cut from it.
2. attention_ref.route, the restatement the GPU tests assert their cases against, agrees with the header for every case of
   tests/test_attention_kernels_gpu.py under every environment that file uses.
3. ops.attention_bwd_takes_q_seq, by which the engine decides whether it may pass out_drop_q_seq, is true exactly where
   attn_bwd_route says attn_bwd3_kernel: Tq, Tk in [1, 320], with and without dropout, under the default environment and each switch.

Row = (name, call, route).  call: op = fwd | bwd (i2t_attention_fwd / i2t_attention_bwd_ex) | gq_fwd | gq_bwd (i2t_gq_attention_*);
B H Hkv hd Tq Tk (Tk = Tq unless given) causal split as in the call; packed: cu_q or cu_k present; drop, od: drop_thr, out_drop_thr
non-zero; q_seq: out_drop_q_seq.  knobs, as attention.hip::attn_knobs parses the variables: v2 (I2T_ATTN_V2 does not start with 0),
bwd (atoi of I2T_ATTN_BWD, 3 unset), bwd2, bwd1 (I2T_ATTN_BWD2 / I2T_ATTN_BWD1 do not start with 0), waves (atoi of
I2T_ATTN_BWD3_WAVES, 0 unset).  route: each launch as kernel<template arguments> grid block, attn_bwd3_kernel with the q_seq it is
handed (0 where out_drop_q_seq equals Tq or there is no out-drop); 'refused out_drop_q_seq' where the call fails instead."""
import os
import re
import shutil
import subprocess

import pytest

import attention_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pair(variant, gq, gkv):
    return f'attn_bwd_dq_kernel<{variant}> grid={gq} block=256 + attn_bwd_dkv_kernel<{variant}> grid={gkv} block=256'


def gq_pair(variant, gq, gkv):
    return f'gattn_bwd_dq_kernel<{variant}> grid={gq} block=256 + gattn_bwd_dkv_kernel<{variant}> grid={gkv} block=256'


REFUSED = 'refused out_drop_q_seq'

TABLE = [
    # ---- forward: Tq 63 | 64, PER 1 .. 4 (112 | 113, 176 | 177, 240 | 241), Tq 304 | 305, Tk 288 | 289, Tk % 4 with dropout
    ('fwd_tq63_tiled', 'op=fwd Tq=63 Tk=64', 'attn_fwd_kernel<false,true> grid=1 block=256'),
    ('fwd_tq64_resident_per1', 'op=fwd Tq=64 Tk=64', 'attn_fwd2_kernel<false,1> grid=1 block=256'),
    ('fwd_tq112_per1', 'op=fwd B=2 H=3 Tq=112 Tk=197', 'attn_fwd2_kernel<false,1> grid=6 block=256'),
    ('fwd_tq113_per2', 'op=fwd B=2 H=3 Tq=113 Tk=197', 'attn_fwd2_kernel<false,2> grid=6 block=256'),
    ('fwd_tq176_per2', 'op=fwd Tq=176 Tk=288', 'attn_fwd2_kernel<false,2> grid=1 block=256'),
    ('fwd_tq177_per3', 'op=fwd Tq=177 Tk=288', 'attn_fwd2_kernel<false,3> grid=1 block=256'),
    ('fwd_tq240_per3', 'op=fwd Tq=240 Tk=9', 'attn_fwd2_kernel<false,3> grid=1 block=256'),
    ('fwd_tq241_per4', 'op=fwd Tq=241 Tk=9', 'attn_fwd2_kernel<false,4> grid=1 block=256'),
    ('fwd_tq304_per4', 'op=fwd B=2 H=2 Tq=304 Tk=288', 'attn_fwd2_kernel<false,4> grid=4 block=256'),
    ('fwd_tq305_tiled', 'op=fwd B=2 H=2 Tq=305 Tk=288', 'attn_fwd_kernel<false,true> grid=20 block=256'),
    ('fwd_tk288_resident', 'op=fwd Tq=197 Tk=288', 'attn_fwd2_kernel<false,3> grid=1 block=256'),
    ('fwd_tk289_tiled', 'op=fwd Tq=197 Tk=289', 'attn_fwd_kernel<false,true> grid=4 block=256'),
    ('fwd_drop_tk196_resident', 'op=fwd Tq=197 Tk=196 drop=1', 'attn_fwd2_kernel<true,3> grid=1 block=256'),
    ('fwd_drop_tk197_tiled_odd', 'op=fwd Tq=197 Tk=197 drop=1', 'attn_fwd_kernel<true,false> grid=4 block=256'),
    ('fwd_drop_tk300_tiled_even', 'op=fwd Tq=197 Tk=300 drop=1', 'attn_fwd_kernel<true,true> grid=4 block=256'),
    ('fwd_drop_tq304', 'op=fwd Tq=304 Tk=64 drop=1', 'attn_fwd2_kernel<true,4> grid=1 block=256'),
    ('fwd_drop_per1', 'op=fwd Tq=64 Tk=64 drop=1', 'attn_fwd2_kernel<true,1> grid=1 block=256'),
    ('fwd_drop_per2', 'op=fwd Tq=113 Tk=196 drop=1', 'attn_fwd2_kernel<true,2> grid=1 block=256'),
    ('fwd_causal_tiled', 'op=fwd B=2 H=2 Tq=130 causal=1', 'attn_fwd_kernel<false,true> grid=12 block=256'),
    ('fwd_causal_drop_odd', 'op=fwd B=2 Tq=130 causal=1 drop=1', 'attn_fwd_kernel<true,false> grid=6 block=256'),
    ('fwd_packed_tiled', 'op=fwd B=5 H=2 Tq=65 packed=1', 'attn_fwd_kernel<false,true> grid=20 block=256'),
    ('fwd_packed_cross_drop', 'op=fwd B=5 H=2 Tq=65 Tk=197 packed=1 drop=1', 'attn_fwd_kernel<true,false> grid=20 block=256'),
    ('fwd_v2_off', 'op=fwd Tq=197 v2=0', 'attn_fwd_kernel<false,true> grid=4 block=256'),
    ('fwd_v2_on', 'op=fwd Tq=197 v2=1', 'attn_fwd2_kernel<false,3> grid=1 block=256'),
    ('fwd_knobs_of_the_backward', 'op=fwd Tq=197 bwd=0 bwd2=0 bwd1=0 waves=9', 'attn_fwd2_kernel<false,3> grid=1 block=256'),
    # ---- backward: Tq 63 | 64, Tq 64 | 65 with Tk <= 64, Tk 64 | 65, Tq 288 | 289, Tq 304 | 305, Tk 288 | 289, Tk % 4 with dropout
    ('bwd_tq63_pair', 'op=bwd Tq=63 Tk=197', pair('false,true', 1, 4)),
    ('bwd_tq64_bwd3', 'op=bwd Tq=64 Tk=197', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_tq63_tk64_bwd1', 'op=bwd Tq=63 Tk=64', 'attn_bwd1_kernel<false,true> grid=1 block=256'),
    ('bwd_tq64_tk64_bwd3', 'op=bwd B=2 H=3 Tq=64 Tk=64', 'attn_bwd3_kernel<false,8> grid=6 block=512 q_seq=0'),
    ('bwd_tq65_tk64_bwd3', 'op=bwd Tq=65 Tk=64', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_tq64_tk64_v2off_bwd1', 'op=bwd B=2 H=3 Tq=64 Tk=64 v2=0', 'attn_bwd1_kernel<false,true> grid=6 block=256'),
    ('bwd_tq65_tk64_v2off_pair', 'op=bwd B=2 H=3 Tq=65 Tk=64 v2=0', pair('false,true', 12, 6)),
    ('bwd_tq40_tk64_bwd1', 'op=bwd Tq=40 Tk=64', 'attn_bwd1_kernel<false,true> grid=1 block=256'),
    ('bwd_tq40_tk65_pair', 'op=bwd Tq=40 Tk=65', pair('false,true', 1, 2)),
    ('bwd_tq288_bwd3', 'op=bwd Tq=288 Tk=197', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_tq289_pair', 'op=bwd Tq=289 Tk=197', pair('false,true', 5, 4)),
    ('bwd_tq304_pair', 'op=bwd B=2 H=2 Tq=304 Tk=288', pair('false,true', 20, 20)),
    ('bwd_tq305_pair', 'op=bwd B=2 H=2 Tq=305 Tk=288', pair('false,true', 20, 20)),
    ('bwd_tk288_bwd3', 'op=bwd Tq=197 Tk=288', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_tk289_pair', 'op=bwd Tq=197 Tk=289', pair('false,true', 4, 5)),
    ('bwd_drop_tk196_bwd3', 'op=bwd Tq=197 Tk=196 drop=1', 'attn_bwd3_kernel<true,8> grid=1 block=512 q_seq=0'),
    ('bwd_drop_tk197_pair_odd', 'op=bwd Tq=197 Tk=197 drop=1', pair('true,false', 4, 4)),
    ('bwd_drop_tk300_pair_even', 'op=bwd Tq=197 Tk=300 drop=1', pair('true,true', 4, 5)),
    ('bwd_drop_tk24_bwd1_even', 'op=bwd Tq=24 drop=1', 'attn_bwd1_kernel<true,true> grid=1 block=256'),
    ('bwd_drop_tk37_bwd1_odd', 'op=bwd Tq=37 causal=1 drop=1', 'attn_bwd1_kernel<true,false> grid=1 block=256'),
    ('bwd_causal_pair', 'op=bwd B=2 H=2 Tq=130 causal=1', pair('false,true', 12, 12)),
    ('bwd_causal_bwd1', 'op=bwd B=2 H=3 Tq=64 causal=1', 'attn_bwd1_kernel<false,true> grid=6 block=256'),
    ('bwd_packed_pair', 'op=bwd B=5 H=2 Tq=65 packed=1', pair('false,true', 20, 20)),
    ('bwd_packed_bwd1', 'op=bwd B=4 H=2 Tq=64 packed=1 drop=1 od=1', 'attn_bwd1_kernel<true,true> grid=8 block=256'),
    ('bwd_packed_cross_pair', 'op=bwd B=5 H=2 Tq=65 Tk=197 packed=1', pair('false,true', 20, 40)),
    # ---- the five variables, every value the code tells apart
    ('bwd_v2_off_pair', 'op=bwd Tq=197 v2=0', pair('false,true', 4, 4)),
    ('bwd_v2_on_bwd3', 'op=bwd Tq=197 v2=1', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_mode3_bwd3', 'op=bwd Tq=197 bwd=3', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_mode2_bwd2', 'op=bwd B=2 Tq=197 bwd=2', 'attn_bwd2_kernel<false> grid=2 block=512'),
    ('bwd_mode2_drop_bwd2', 'op=bwd Tq=197 Tk=272 bwd=2 drop=1', 'attn_bwd2_kernel<true> grid=1 block=512'),
    ('bwd_mode1_bwd2', 'op=bwd Tq=197 bwd=1', 'attn_bwd2_kernel<false> grid=1 block=512'),
    ('bwd_mode4_bwd2', 'op=bwd Tq=197 bwd=4', 'attn_bwd2_kernel<false> grid=1 block=512'),
    ('bwd_mode0_pair', 'op=bwd Tq=197 bwd=0', pair('false,true', 4, 4)),
    ('bwd_mode2_tq289_pair', 'op=bwd Tq=289 Tk=197 bwd=2', pair('false,true', 5, 4)),
    ('bwd_mode0_single_tile_bwd1', 'op=bwd Tq=64 Tk=16 bwd=0', 'attn_bwd1_kernel<false,true> grid=1 block=256'),
    ('bwd_bwd2_off_pair', 'op=bwd Tq=197 bwd2=0', pair('false,true', 4, 4)),
    ('bwd_bwd2_off_beats_mode2', 'op=bwd Tq=197 bwd=2 bwd2=0', pair('false,true', 4, 4)),
    ('bwd_bwd2_on_bwd3', 'op=bwd Tq=197 bwd2=1', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_bwd1_off_pair', 'op=bwd Tq=24 bwd1=0', pair('false,true', 1, 1)),
    ('bwd_bwd1_off_drop_odd', 'op=bwd B=2 Tq=5 Tk=9 drop=1 bwd1=0', pair('true,false', 2, 2)),
    ('bwd_bwd1_on', 'op=bwd Tq=24 bwd1=1', 'attn_bwd1_kernel<false,true> grid=1 block=256'),
    ('bwd_waves9', 'op=bwd B=2 Tq=197 waves=9', 'attn_bwd3_kernel<false,9> grid=2 block=576 q_seq=0'),
    ('bwd_waves9_drop', 'op=bwd Tq=288 Tk=288 drop=1 od=1 waves=9', 'attn_bwd3_kernel<true,9> grid=1 block=576 q_seq=0'),
    ('bwd_waves8', 'op=bwd Tq=197 waves=8', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_waves7_is_8', 'op=bwd Tq=197 waves=7', 'attn_bwd3_kernel<false,8> grid=1 block=512 q_seq=0'),
    ('bwd_waves9_off_bwd3', 'op=bwd Tq=197 bwd=2 waves=9', 'attn_bwd2_kernel<false> grid=1 block=512'),
    # ---- out_drop_q_seq: accepted, normalised away, refused
    ('qseq_accepted', 'op=bwd B=2 H=2 Tq=64 Tk=197 od=1 q_seq=197', 'attn_bwd3_kernel<false,8> grid=4 block=512 q_seq=197'),
    ('qseq_accepted_drop', 'op=bwd B=2 H=2 Tq=64 Tk=196 od=1 q_seq=196 drop=1', 'attn_bwd3_kernel<true,8> grid=4 block=512 q_seq=196'),
    ('qseq_equals_tq', 'op=bwd B=2 H=2 Tq=64 Tk=197 od=1 q_seq=64', 'attn_bwd3_kernel<false,8> grid=4 block=512 q_seq=0'),
    ('qseq_without_out_drop', 'op=bwd B=2 H=2 Tq=64 Tk=197 q_seq=197', 'attn_bwd3_kernel<false,8> grid=4 block=512 q_seq=0'),
    ('qseq_without_out_drop_bwd1', 'op=bwd Tq=40 q_seq=197', 'attn_bwd1_kernel<false,true> grid=1 block=256'),
    ('qseq_refused_mode2', 'op=bwd B=2 H=2 Tq=64 Tk=197 od=1 q_seq=197 bwd=2', REFUSED),
    ('qseq_refused_mode0', 'op=bwd B=2 H=2 Tq=64 Tk=197 od=1 q_seq=197 bwd=0', REFUSED),
    ('qseq_refused_bwd1', 'op=bwd Tq=40 od=1 q_seq=197', REFUSED),
    ('qseq_refused_pair_tk289', 'op=bwd Tq=64 Tk=289 od=1 q_seq=289', REFUSED),
    ('qseq_refused_v2_off', 'op=bwd Tq=64 Tk=197 od=1 q_seq=197 v2=0', REFUSED),
    # ---- grouped-query heads: hd 16, 32, 64, 128, with and without dropout, split
    ('gq_fwd_hd16', 'op=gq_fwd B=2 H=8 Hkv=1 hd=16 Tq=70 causal=1', 'gattn_fwd_kernel<32,false> grid=32 block=256'),
    ('gq_fwd_hd16_drop', 'op=gq_fwd B=2 H=4 Hkv=2 hd=16 Tq=40 Tk=37 drop=1', 'gattn_fwd_kernel<32,true> grid=8 block=256'),
    ('gq_fwd_hd32', 'op=gq_fwd H=4 Hkv=2 hd=32 Tq=257', 'gattn_fwd_kernel<32,false> grid=20 block=256'),
    ('gq_fwd_hd32_drop', 'op=gq_fwd H=4 Hkv=2 hd=32 Tq=257 drop=1', 'gattn_fwd_kernel<32,true> grid=20 block=256'),
    ('gq_fwd_hd64', 'op=gq_fwd B=2 H=2 Hkv=2 hd=64 Tq=65 causal=1', 'gattn_fwd_kernel<64,false> grid=8 block=256'),
    ('gq_fwd_hd64_drop', 'op=gq_fwd H=8 Hkv=1 hd=64 Tq=70 Tk=37 drop=1', 'gattn_fwd_kernel<64,true> grid=16 block=256'),
    ('gq_fwd_hd128', 'op=gq_fwd B=2 H=2 Hkv=2 hd=128 Tq=64 Tk=130', 'gattn_fwd_kernel<128,false> grid=4 block=256'),
    ('gq_fwd_hd128_drop', 'op=gq_fwd H=2 Hkv=1 hd=128 Tq=100 Tk=131 drop=1', 'gattn_fwd_kernel<128,true> grid=4 block=256'),
    ('gq_fwd_split_hd32', 'op=gq_fwd B=2 H=4 Hkv=2 hd=32 Tq=96 split=63', 'gattn_fwd_kernel<32,false> grid=16 block=256'),
    ('gq_fwd_split_hd64_drop', 'op=gq_fwd H=2 Hkv=1 hd=64 Tq=130 split=65 drop=1', 'gattn_fwd_kernel<64,true> grid=6 block=256'),
    ('gq_fwd_packed', 'op=gq_fwd B=5 H=4 Hkv=2 hd=32 Tq=65 packed=1 causal=1', 'gattn_fwd_kernel<32,false> grid=40 block=256'),
    ('gq_fwd_ignores_the_knobs', 'op=gq_fwd H=4 Hkv=2 hd=64 Tq=197 v2=0 bwd=0 bwd2=0 bwd1=0 waves=9', 'gattn_fwd_kernel<64,false> grid=16 block=256'),
    ('gq_bwd_hd16', 'op=gq_bwd B=2 H=8 Hkv=1 hd=16 Tq=70 causal=1', gq_pair('32,false', 32, 4)),
    ('gq_bwd_hd16_drop', 'op=gq_bwd B=2 H=4 Hkv=2 hd=16 Tq=40 Tk=37 drop=1', gq_pair('32,true', 8, 4)),
    ('gq_bwd_hd32', 'op=gq_bwd H=4 Hkv=2 hd=32 Tq=257', gq_pair('32,false', 20, 10)),
    ('gq_bwd_hd32_drop', 'op=gq_bwd H=4 Hkv=2 hd=32 Tq=257 drop=1', gq_pair('32,true', 20, 10)),
    ('gq_bwd_hd64', 'op=gq_bwd B=2 H=2 Hkv=2 hd=64 Tq=65 causal=1', gq_pair('64,false', 8, 8)),
    ('gq_bwd_hd64_drop', 'op=gq_bwd H=8 Hkv=1 hd=64 Tq=70 Tk=37 drop=1 od=1', gq_pair('64,true', 16, 1)),
    ('gq_bwd_hd128', 'op=gq_bwd B=2 H=2 Hkv=2 hd=128 Tq=64 Tk=130', gq_pair('128,false', 4, 12)),
    ('gq_bwd_hd128_drop', 'op=gq_bwd H=2 Hkv=1 hd=128 Tq=100 Tk=131 drop=1 od=1', gq_pair('128,true', 4, 3)),
    ('gq_bwd_packed_cross', 'op=gq_bwd B=4 H=8 Hkv=1 hd=64 Tq=65 Tk=130 packed=1', gq_pair('64,false', 64, 12)),
]


@pytest.fixture(scope='module')
def route_cli(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler found (set CXX)'
    exe = str(tmp_path_factory.mktemp('attention_route') / 'attention_route_cli')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', os.path.join(ROOT, 'tests', 'attention_route_cli.cpp'), '-o', exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def routes(exe, calls):
    """{name: route} of (name, call) pairs"""
    r = subprocess.run([exe], input=''.join(f'{name} {call}\n' for name, call in calls), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    return dict(line.split(' ', 1) for line in r.stdout.splitlines())


def test_routes_match_the_recorded_table(route_cli):
    got = routes(route_cli, [(name, call) for name, call, _ in TABLE])
    wrong = [f'{name}: {call}\n    expected {route}\n    got      {got.get(name)}' for name, call, route in TABLE if got.get(name) != route]
    assert not wrong, 'routes changed:\n  ' + '\n  '.join(wrong)


def test_the_table_covers_every_route_kind_and_knob():
    names = [name for name, _, _ in TABLE]
    assert len(set(names)) == len(names)
    text = ' '.join(route for _, _, route in TABLE)
    for kernel in ([f'attn_fwd2_kernel<{d},{per}>' for d in ('false', 'true') for per in (1, 2, 3, 4)] +
                   [f'{k}<{v}>' for k in ('attn_fwd_kernel', 'attn_bwd1_kernel', 'attn_bwd_dq_kernel', 'attn_bwd_dkv_kernel')
                    for v in ('false,true', 'true,true', 'true,false')] +
                   [f'attn_bwd3_kernel<{d},{w}>' for d in ('false', 'true') for w in (8, 9)] + ['attn_bwd2_kernel<false>', 'attn_bwd2_kernel<true>'] +
                   [f'{k}<{d},{drop}>' for k in ('gattn_fwd_kernel', 'gattn_bwd_dq_kernel', 'gattn_bwd_dkv_kernel') for d in (32, 64, 128)
                    for drop in ('false', 'true')] + [REFUSED, 'q_seq=0', 'q_seq=197']):
        assert kernel in text, kernel
    calls = [call for _, call, _ in TABLE]
    for field in ('op=fwd', 'op=bwd', 'op=gq_fwd', 'op=gq_bwd', 'causal=1', 'packed=1', 'drop=1', 'od=1', 'split=', 'hd=16', 'hd=32', 'hd=64', 'hd=128',
                  'v2=0', 'v2=1', 'bwd=0', 'bwd=1', 'bwd=2', 'bwd=3', 'bwd2=0', 'bwd2=1', 'bwd1=0', 'bwd1=1', 'waves=8', 'waves=9'):
        assert any(f' {field}' in f' {call}' for call in calls), field
    # both sides of every boundary of the rule, in both directions where both have it
    sizes = {(op, int(re.search(r'Tq=(\d+)', call).group(1)), int((re.search(r'Tk=(\d+)', call) or re.search(r'Tq=(\d+)', call)).group(1)))
             for call in calls for op in re.findall(r'op=(fwd|bwd)\b', call)}
    for op in ('fwd', 'bwd'):
        for tq in (63, 64, 304, 305):
            assert any(o == op and q == tq for o, q, _ in sizes), (op, 'Tq', tq)
        for tk in (288, 289):
            assert any(o == op and k == tk for o, _, k in sizes), (op, 'Tk', tk)
    for tq in (112, 113, 176, 177, 240, 241):
        assert any(o == 'fwd' and q == tq for o, q, _ in sizes), ('fwd', 'Tq', tq)
    for tq, tk in ((64, 64), (65, 64), (40, 64), (40, 65), (288, 197), (289, 197)):
        assert ('bwd', tq, tk) in sizes, ('bwd', tq, tk)
    for op in ('fwd', 'bwd'):
        rem = {int((re.search(r'Tk=(\d+)', call) or re.search(r'Tq=(\d+)', call)).group(1)) % 4 != 0 for call in calls if f'op={op} ' in call and 'drop=1' in call.split()}
        assert rem == {False, True}, (op, 'Tk % 4 with dropout')


# ---------------------------------------------------------------------------------------------- attention_ref.route against the header
def knobs(env):
    """the CLI's knob fields for an environment, parsed as attention.hip::attn_knobs parses it"""
    on = lambda name: int(env.get(name, '1')[:1] != '0')
    return (f"v2={on('I2T_ATTN_V2')} bwd={int(env.get('I2T_ATTN_BWD', '3'))} bwd2={on('I2T_ATTN_BWD2')} bwd1={on('I2T_ATTN_BWD1')} "
            f"waves={int(env.get('I2T_ATTN_BWD3_WAVES', '0'))}")


def call_of(c, op):
    return (f'op={op} B={c.B} H={c.H} Hkv={c.Hkv} hd={c.hd} Tq={c.Tq} Tk={c.Tk} causal={int(c.causal)} packed={int(c.lens is not None)} drop={int(c.drop)} '
            f'od={int(c.od)} q_seq={c.q_seq} split={c.split if op == "gq_fwd" else 0}')


VARIANT = {'false,true': 'nodrop', 'true,true': 'even', 'true,false': 'odd'}


def host_part(route):
    """a CLI route in the words of attention_ref.route, as far as the host decides it: kernel, PER, NWV and drop variant -> (text, DROP)"""
    kernels = re.findall(r'(\w+)_kernel<([^>]*)>', route)
    name, targs = kernels[0]
    if name == 'attn_fwd2':
        return f'fwd2<PER={targs.split(",")[1]}>', targs.split(',')[0]
    if name == 'attn_fwd':
        return f'fwd<{VARIANT[targs]}>', targs.split(',')[0]
    if name == 'attn_bwd3':
        return f'bwd3<{targs.split(",")[1]}', targs.split(',')[0]
    if name == 'attn_bwd2':
        return 'bwd2', targs
    if name == 'attn_bwd1':
        return f'bwd1<{VARIANT[targs]}>', targs.split(',')[0]
    assert [k for k, _ in kernels] == ['attn_bwd_dq', 'attn_bwd_dkv'] and kernels[0][1] == kernels[1][1], route
    return f'pair<{VARIANT[targs]}>', targs.split(',')[0]


def test_the_python_restatement_agrees_with_the_header(route_cli):
    """every head_dim-64 case of the GPU file under every environment it runs a case in; CNT of bwd3<NWV,CNT=..> is the kernel's own"""
    envs = [{}] + [env for env, _ in A.SWITCHES.values()] + [{'I2T_ATTN_BWD1': '0'}]
    assert all(set(env) <= set(A.ENVS) for env in envs)
    cases = {c.id: c for c in A.FWD_TILED + A.FWD_V2 + A.BWD3 + A.BWD3_QSEQ + A.BWD1 + A.PAIR}
    assert len(cases) > 150
    calls = [(f'{cid}|{e}|{op}', f'{call_of(c, op)} {knobs(env)}') for cid, c in cases.items() for e, env in enumerate(envs) for op in ('fwd', 'bwd')]
    got = routes(route_cli, calls)
    assert len(got) == len(calls)
    for cid, c in cases.items():
        for e, env in enumerate(envs):
            fwd, bwd = A.route(c, env)
            text, drop = host_part(got[f'{cid}|{e}|fwd'])
            assert (text, drop) == (fwd, str(c.drop).lower()), (cid, env, got[f'{cid}|{e}|fwd'], fwd)
            q_seq = c.q_seq if c.od and c.q_seq != c.Tq else 0
            if got[f'{cid}|{e}|bwd'] == REFUSED:                 # (test_q_seq_is_refused_off_the_one_pass_kernel runs two of these)
                assert q_seq and not bwd.startswith('bwd3'), (cid, env, bwd)
                continue
            assert not q_seq or bwd.startswith('bwd3'), (cid, env, bwd)
            text, drop = host_part(got[f'{cid}|{e}|bwd'])
            assert (text, drop) == (re.sub(r',CNT=\d+>$', '', bwd), str(c.drop).lower()), (cid, env, got[f'{cid}|{e}|bwd'], bwd)
            if bwd.startswith('bwd3'):
                assert got[f'{cid}|{e}|bwd'].endswith(f' q_seq={q_seq}')


def test_the_grouped_cases_take_the_instantiation_of_their_head_width(route_cli):
    cases = {c.id: c for c in A.GQ + A.GQ_SPLIT}
    got = routes(route_cli, [(f'{cid}|{op}', call_of(c, op)) for cid, c in cases.items() for op in ('gq_fwd', 'gq_bwd')])
    for cid, c in cases.items():
        targs = f'<{ {16: 32, 32: 32, 64: 64, 128: 128}[c.hd]},{str(c.drop).lower()}>'
        assert got[f'{cid}|gq_fwd'].startswith(f'gattn_fwd_kernel{targs} '), (cid, got[f'{cid}|gq_fwd'])
        assert re.findall(r'(\w+<[^>]*>)', got[f'{cid}|gq_bwd']) == [f'gattn_bwd_dq_kernel{targs}', f'gattn_bwd_dkv_kernel{targs}'], (cid, got[f'{cid}|gq_bwd'])


# ------------------------------------------------------------------------------ ops.attention_bwd_takes_q_seq against attn_bwd_route
Q_SEQ_ENVS = [{}, {'I2T_ATTN_V2': '0'}, {'I2T_ATTN_V2': '1'}, {'I2T_ATTN_BWD': '0'}, {'I2T_ATTN_BWD': '2'}, {'I2T_ATTN_BWD': '3'}, {'I2T_ATTN_BWD2': '0'},
              {'I2T_ATTN_BWD2': '1'}, {'I2T_ATTN_BWD1': '0'}, {'I2T_ATTN_BWD3_WAVES': '8'}, {'I2T_ATTN_BWD3_WAVES': '9'}]


@pytest.mark.parametrize('env', Q_SEQ_ENVS, ids=lambda env: '-'.join(f'{k[4:]}={v}' for k, v in env.items()) or 'default')
def test_takes_q_seq_is_the_bwd3_route(route_cli, env, monkeypatch):
    """dense non-causal calls, Tq, Tk in [1, 320], with and without dropout"""
    from image2text_amd import ops
    for name in A.ENVS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    grid = [(tq, tk, drop) for tq in range(1, 321) for tk in range(1, 321) for drop in (0, 1)]
    got = routes(route_cli, [(f'{tq},{tk},{drop}', f'op=bwd Tq={tq} Tk={tk} drop={drop} {knobs(env)}') for tq, tk, drop in grid])
    assert len(got) == len(grid)
    wrong = [(tq, tk, drop) for tq, tk, drop in grid
             if ops.attention_bwd_takes_q_seq(tq, tk, (1, 7, 1000, 1.0) if drop else None) != got[f'{tq},{tk},{drop}'].startswith('attn_bwd3_kernel<')]
    assert not wrong, f'{len(wrong)} calls, the first {wrong[:5]}'
