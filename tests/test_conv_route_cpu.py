"""Which kernels a convolution call reaches (image2text_amd/csrc/conv_route.h), checked on the CPU: tests/conv_route_cli.cpp is compiled
with the host C++ compiler (no HIP), fed calls and must print the launches they make.  The checks:

1. TABLE.  The expected launches were recorded from the host code of csrc/conv_mfma.hip and csrc/conv.hip as it stood BEFORE the rule
   moved into conv_route.h (that code copied -- conv_mfma_dispatch, the LAUNCH_CONV / LAUNCH_BW / BWD_W_CASE macros, dispatch_cout,
   launch_direct and the seven entry points -- with every hipLaunchKernelGGL / hipMemsetAsync replaced by a recorder of kernel name,
   template arguments, grid, block and the integer arguments), not read off conv_route.h: a row that fails says the routing changed.
   The same recorder agreed with conv_route.h, launch for launch and refusal text for refusal text (after the entry point's name), on
   the whole grid op x x_layout, dy_layout in {0, 1, 2} x in_gelu x dst_nchw x pre-activation present / absent x Cin, Cout in [1, 34]
   x (H, W) in {(1, 1), (16, 16), (17, 33), (16, 132)} x B in {1, 3} x deterministic mode off / on, the generic path with in_is_f32
   in {0, 1, 2} and k in {3, 4, 5, 6}, the transpose with C in [1, 34] and each pointer aligned or not, before the table was cut
   from it: 6 659 648 calls, 907 648 of them accepted, 0 differences.
2. What changed on purpose is not in the table: a call with H = 0 or W = 0 (and, on the entry points that did not ask, Cin = 0 or
   Cout = 0) is refused with 'bad args' by the one conv_check instead of reaching a launch with an empty grid.
3. conv_ref.route / transpose_route, the restatement the GPU tests assert their cases against, agree with the header for every case
   of tests/test_conv_kernels_gpu.py, and conv_ref.all_routes() is the set the *_instantiated predicates state.
4. ops.conv_stack_takes_mfma, by which the engine decides which entry points a ConvMLP stack takes, says MFMA only where the header
   accepts every call encode / encode_backward then make; ops.CONV6_WS_ELEMS / CONV6_SCRATCH_FLOATS cover what the routes ask for.

Row = (name, call, route).  call: op = fwd | bwd_data | bwd_weight | transpose (i2t_conv6_* / i2t_nchw_to_nhwc_bf16) | gfwd |
gbwd_data | gbwd_weight (i2t_conv_*, the generic path); xl, dyl: x_layout, dy_layout (0 fp32 NCHW, 1 bf16 NCHW, 2 bf16 NHWC); f32:
in_is_f32 of the generic path; gelu: in_gelu; nchw: y_nchw; pre: x_pre present; B Cin Cout H W k as in the call (transpose: C);
aligned: both pointers of the transpose 16-byte aligned; det: deterministic mode; ptr=0: a required pointer is null.  route: each
launch as kernel<template arguments> grid block args=(its integer arguments in order), 'memset bytes=' for the scratch memset;
'refused: text' where the call fails instead.  conv_mfma_kernel<CP, NT, SRC, IN_GELU, DGELU, DST_NCHW, NW, GRP>;
conv_mfma_bwd_weight_kernel<CP, COP, DY_SRC, ACT_SRC, ACT_GELU>; conv_direct_kernel<COUT_T, K, IN_F32, IN_GELU, DGELU>;
conv_bwd_weight_kernel<COUT, K, IN_F32, IN_GELU>."""
import itertools
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = [
    # ---- forward, the fp32 image: Cin 4 | 5 (the staging inside the kernel changes there: chunks | planar), 8 | 9, Cout 16 | 17, 32 | 33, both outputs
    ('fwd_img_cin3', 'op=fwd xl=0 Cin=3 Cout=8 B=3 H=17 W=33',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(8,3,16,8,0) + conv_mfma_kernel<8,1,0,false,false,false,4,1> grid=(2,3,1) block=256 args=(3,8,17,33,2,3)'),
    ('fwd_img_cin4_chunks', 'op=fwd xl=0 Cin=4 Cout=16',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,4,16,8,0) + conv_mfma_kernel<8,1,0,false,false,false,4,1> grid=(1,1,1) block=256 args=(4,16,16,16,2,1)'),
    ('fwd_img_cin5_planar', 'op=fwd xl=0 Cin=5 Cout=16',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,5,16,8,0) + conv_mfma_kernel<8,1,0,false,false,false,4,1> grid=(1,1,1) block=256 args=(5,16,16,16,2,1)'),
    ('fwd_img_cin8', 'op=fwd xl=0 Cin=8 Cout=16',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,8,16,8,0) + conv_mfma_kernel<8,1,0,false,false,false,4,1> grid=(1,1,1) block=256 args=(8,16,16,16,2,1)'),
    ('fwd_img_cin9_refused', 'op=fwd xl=0 Cin=9 Cout=16 nchw=1',
     'refused: unsupported layout combination (src=0 gelu=0 dgelu=0 nchw_out=1)'),
    ('fwd_img_cout17', 'op=fwd xl=0 Cin=3 Cout=17 nchw=1',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(17,3,32,8,0) + conv_mfma_kernel<8,2,0,false,false,true,4,1> grid=(1,1,1) block=256 args=(3,17,16,16,2,1)'),
    ('fwd_img_cout24_nhwc', 'op=fwd xl=0 Cin=3 Cout=24',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(24,3,32,8,0) + conv_mfma_kernel<8,2,0,false,false,false,4,1> grid=(1,1,1) block=256 args=(3,24,16,16,2,1)'),
    ('fwd_img_cout16_nchw', 'op=fwd xl=0 Cin=3 Cout=16 nchw=1',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,3,16,8,0) + conv_mfma_kernel<8,1,0,false,false,true,4,1> grid=(1,1,1) block=256 args=(3,16,16,16,2,1)'),
    ('fwd_img_cout32_nchw', 'op=fwd xl=0 Cin=8 Cout=32 nchw=1 B=3 H=16 W=132',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(32,8,32,8,0) + conv_mfma_kernel<8,2,0,false,false,true,4,1> grid=(1,3,1) block=256 args=(8,32,16,132,2,9)'),
    ('fwd_img_cout33_refused', 'op=fwd xl=0 Cin=3 Cout=33 nchw=1',
     'refused: bad args'),
    ('fwd_img_gelu_refused', 'op=fwd xl=0 gelu=1 Cin=3 Cout=16 nchw=1',
     'refused: unsupported layout combination (src=0 gelu=1 dgelu=0 nchw_out=1)'),
    ('fwd_img_cout20_nhwc_refused', 'op=fwd xl=0 Cin=3 Cout=20',
     'refused: NHWC output needs Cout % 8 == 0'),
    # ---- forward, NHWC through GELU: Cin 8, 16, 32 | 33, Cout 16 | 17, 32 | 33, Cout % 8 with NHWC in and out, tiles_x 1 and 9, NW and GRP
    ('fwd_nhwc_cin8_cout16', 'op=fwd xl=2 gelu=1 Cin=8 Cout=16',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,8,16,8,0) + conv_mfma_kernel<8,1,2,true,false,false,4,1> grid=(1,1,1) block=256 args=(8,16,16,16,2,1)'),
    ('fwd_nhwc_cin8_cout24', 'op=fwd xl=2 gelu=1 Cin=8 Cout=24 H=17 W=33',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(24,8,32,8,0) + conv_mfma_kernel<8,2,2,true,false,false,4,1> grid=(2,1,1) block=256 args=(8,24,17,33,2,3)'),
    ('fwd_nhwc_cin8_cout20_refused', 'op=fwd xl=2 gelu=1 Cin=8 Cout=20',
     'refused: NHWC output needs Cout % 8 == 0'),
    ('fwd_nhwc_cin8_cout5_nchw', 'op=fwd xl=2 gelu=1 Cin=8 Cout=5 nchw=1 H=17 W=33',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(5,8,16,8,0) + conv_mfma_kernel<8,1,2,true,false,true,4,1> grid=(2,1,1) block=256 args=(8,5,17,33,2,3)'),
    ('fwd_nhwc_cin8_cout17_nchw', 'op=fwd xl=2 gelu=1 Cin=8 Cout=17 nchw=1',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(17,8,32,8,0) + conv_mfma_kernel<8,2,2,true,false,true,4,1> grid=(1,1,1) block=256 args=(8,17,16,16,2,1)'),
    ('fwd_nhwc_cin16_cout16', 'op=fwd xl=2 gelu=1 Cin=16 Cout=16',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,16,16,16,0) + conv_mfma_kernel<16,1,2,true,false,false,4,1> grid=(1,1,1) block=256 args=(16,16,16,16,2,1)'),
    ('fwd_nhwc_cin16_cout32', 'op=fwd xl=2 gelu=1 Cin=16 Cout=32 B=3',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(32,16,32,16,0) + conv_mfma_kernel<16,2,2,true,false,false,4,1> grid=(1,3,1) block=256 args=(16,32,16,16,2,1)'),
    ('fwd_nhwc_cin16_cout32_nchw_tiles9', 'op=fwd xl=2 gelu=1 Cin=16 Cout=32 nchw=1 B=3 H=16 W=132',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(32,16,32,16,0) + conv_mfma_kernel<16,2,2,true,false,true,8,4> grid=(1,3,1) block=512 args=(16,32,16,132,2,9)'),
    ('fwd_nhwc_cin16_cout5_nchw_tiles1', 'op=fwd xl=2 gelu=1 Cin=16 Cout=5 nchw=1 H=1 W=1',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(5,16,16,16,0) + conv_mfma_kernel<16,1,2,true,false,true,8,4> grid=(1,1,1) block=512 args=(16,5,1,1,2,1)'),
    ('fwd_nhwc_cin32_cout16', 'op=fwd xl=2 gelu=1 Cin=32 Cout=16 H=17 W=33',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,32,16,32,0) + conv_mfma_kernel<32,1,2,true,false,false,8,1> grid=(2,1,1) block=512 args=(32,16,17,33,2,3)'),
    ('fwd_nhwc_cin32_cout32', 'op=fwd xl=2 gelu=1 Cin=32 Cout=32',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(32,32,32,32,0) + conv_mfma_kernel<32,2,2,true,false,false,8,1> grid=(1,1,1) block=512 args=(32,32,16,16,2,1)'),
    ('fwd_nhwc_cin32_cout16_nchw', 'op=fwd xl=2 gelu=1 Cin=32 Cout=16 nchw=1',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,32,16,32,0) + conv_mfma_kernel<32,1,2,true,false,true,8,4> grid=(1,1,1) block=512 args=(32,16,16,16,2,1)'),
    ('fwd_nhwc_cin32_cout17_nchw', 'op=fwd xl=2 gelu=1 Cin=32 Cout=17 nchw=1 W=132',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(17,32,32,32,0) + conv_mfma_kernel<32,2,2,true,false,true,8,4> grid=(1,1,1) block=512 args=(32,17,16,132,2,9)'),
    ('fwd_nhwc_cin33_refused', 'op=fwd xl=2 gelu=1 Cin=33 Cout=16 nchw=1',
     'refused: bad args'),
    ('fwd_nhwc_cout33_refused', 'op=fwd xl=2 gelu=1 Cin=16 Cout=33 nchw=1',
     'refused: bad args'),
    ('fwd_nhwc_cin9_refused', 'op=fwd xl=2 gelu=1 Cin=9 Cout=16',
     'refused: NHWC input needs 8/16/32 channels'),
    ('fwd_nhwc_cin17_refused', 'op=fwd xl=2 gelu=1 Cin=17 Cout=16',
     'refused: NHWC input needs 8/16/32 channels'),
    ('fwd_nhwc_cout12_refused', 'op=fwd xl=2 gelu=1 Cin=16 Cout=12',
     'refused: NHWC output needs Cout % 8 == 0'),
    ('fwd_nhwc_without_gelu_refused', 'op=fwd xl=2 gelu=0 Cin=8 Cout=16 nchw=1',
     'refused: unsupported layout combination (src=2 gelu=0 dgelu=0 nchw_out=1)'),
    ('fwd_nchw_bf16_refused', 'op=fwd xl=1 gelu=0 Cin=8 Cout=16 nchw=1',
     'refused: unsupported layout combination (src=1 gelu=0 dgelu=0 nchw_out=1)'),
    ('fwd_null_pointer_refused', 'op=fwd xl=0 Cin=3 Cout=16 ptr=0',
     'refused: bad args'),
    # ---- backward-data: dY NCHW | NHWC, Cout 8 | 9, 16 | 17, 32 | 33, Cin 8 | 16, mirrored padding, flipped repack
    ('bwd_data_nchw_cout8', 'op=bwd_data dyl=1 Cin=8 Cout=8',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(8,8,16,8,1) + conv_mfma_kernel<8,1,1,false,true,false,4,1> grid=(1,1,1) block=256 args=(8,8,16,16,3,1)'),
    ('bwd_data_nchw_cout9', 'op=bwd_data dyl=1 Cin=8 Cout=9',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(9,8,16,16,1) + conv_mfma_kernel<16,1,1,false,true,false,4,1> grid=(1,1,1) block=256 args=(9,8,16,16,3,1)'),
    ('bwd_data_nchw_cout16', 'op=bwd_data dyl=1 Cin=16 Cout=16 B=3 H=17 W=33',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,16,16,16,1) + conv_mfma_kernel<16,1,1,false,true,false,4,1> grid=(2,3,1) block=256 args=(16,16,17,33,3,3)'),
    ('bwd_data_nchw_cout17', 'op=bwd_data dyl=1 Cin=16 Cout=17',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(17,16,16,32,1) + conv_mfma_kernel<32,1,1,false,true,false,8,1> grid=(1,1,1) block=512 args=(17,16,16,16,3,1)'),
    ('bwd_data_nchw_cout32', 'op=bwd_data dyl=1 Cin=16 Cout=32',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(32,16,16,32,1) + conv_mfma_kernel<32,1,1,false,true,false,8,1> grid=(1,1,1) block=512 args=(32,16,16,16,3,1)'),
    ('bwd_data_nhwc_cout8', 'op=bwd_data dyl=2 Cin=8 Cout=8',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(8,8,16,8,1) + conv_mfma_kernel<8,1,2,false,true,false,4,1> grid=(1,1,1) block=256 args=(8,8,16,16,3,1)'),
    ('bwd_data_nhwc_cout16', 'op=bwd_data dyl=2 Cin=8 Cout=16 W=132',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(16,8,16,16,1) + conv_mfma_kernel<16,1,2,false,true,false,4,1> grid=(1,1,1) block=256 args=(16,8,16,132,3,9)'),
    ('bwd_data_nhwc_cout32', 'op=bwd_data dyl=2 Cin=16 Cout=32 B=3 H=16 W=132',
     'conv_repack_kernel grid=(64,1,1) block=256 args=(32,16,16,32,1) + conv_mfma_kernel<32,1,2,false,true,false,8,1> grid=(1,3,1) block=512 args=(32,16,16,132,3,9)'),
    ('bwd_data_cout33_refused', 'op=bwd_data dyl=2 Cin=16 Cout=33',
     'refused: bad args'),
    ('bwd_data_cin17_refused', 'op=bwd_data dyl=2 Cin=17 Cout=32',
     'refused: bad args'),
    ('bwd_data_cin24_refused', 'op=bwd_data dyl=2 Cin=24 Cout=32',
     'refused: bad args'),
    ('bwd_data_cin32_refused', 'op=bwd_data dyl=2 Cin=32 Cout=32',
     'refused: bad args'),
    ('bwd_data_cin12_refused', 'op=bwd_data dyl=2 Cin=12 Cout=32',
     'refused: bad args'),
    ('bwd_data_without_pre_refused', 'op=bwd_data dyl=2 Cin=16 Cout=32 pre=0',
     'refused: bad args'),
    ('bwd_data_nhwc_cout24_refused', 'op=bwd_data dyl=2 Cin=16 Cout=24',
     'refused: dy layout'),
    ('bwd_data_f32_dy_refused', 'op=bwd_data dyl=0 Cin=16 Cout=32',
     'refused: dy layout'),
    # ---- backward-weight: image Cin 4 | 5, 8 | 9; NHWC Cin 8, 16 | 17; Cout 16 | 17, 32 | 33; dY NCHW | NHWC; deterministic mode off | on
    ('bwd_weight_img_cin4_chunks', 'op=bwd_weight xl=0 dyl=2 Cin=4 Cout=8',
     'memset bytes=18432 + conv_mfma_bwd_weight_kernel<8,16,2,0,false> grid=(1,1,1) block=256 args=(4,8,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(8,4,8)'),
    ('bwd_weight_img_cin5_planar', 'op=bwd_weight xl=0 dyl=2 Cin=5 Cout=24',
     'memset bytes=36864 + conv_mfma_bwd_weight_kernel<8,32,2,0,false> grid=(1,1,1) block=256 args=(5,24,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(24,5,8)'),
    ('bwd_weight_img_cin8_nchw_dy', 'op=bwd_weight xl=0 dyl=1 Cin=8 Cout=16',
     'memset bytes=18432 + conv_mfma_bwd_weight_kernel<8,16,1,0,false> grid=(1,1,1) block=256 args=(8,16,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(16,8,8)'),
    ('bwd_weight_img_nchw_dy_cout17', 'op=bwd_weight xl=0 dyl=1 Cin=3 Cout=17 B=3 H=17 W=33',
     'memset bytes=36864 + conv_mfma_bwd_weight_kernel<8,32,1,0,false> grid=(2,3,1) block=256 args=(3,17,17,33,2,3,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(17,3,8)'),
    ('bwd_weight_img_cin9_refused', 'op=bwd_weight xl=0 dyl=2 Cin=9 Cout=16',
     'refused: unsupported layout combination (x_layout=0 gelu=0 Cin=9)'),
    ('bwd_weight_img_gelu_refused', 'op=bwd_weight xl=0 gelu=1 dyl=2 Cin=3 Cout=16',
     'refused: unsupported layout combination (x_layout=0 gelu=1 Cin=3)'),
    ('bwd_weight_img_det', 'op=bwd_weight xl=0 dyl=1 Cin=3 Cout=8 B=3 H=17 W=33 det=1',
     'memset bytes=18432 + conv_mfma_bwd_weight_kernel<8,16,1,0,false> grid=(1,1,1) block=256 args=(3,8,17,33,2,3,0,0) + conv_mfma_bwd_weight_kernel<8,16,1,0,false> grid=(1,1,1) block=256 args=(3,8,17,33,2,3,1,0) + conv_mfma_bwd_weight_kernel<8,16,1,0,false> grid=(1,1,1) block=256 args=(3,8,17,33,2,3,0,1) + conv_mfma_bwd_weight_kernel<8,16,1,0,false> grid=(1,1,1) block=256 args=(3,8,17,33,2,3,1,1) + conv_mfma_bwd_weight_kernel<8,16,1,0,false> grid=(1,1,1) block=256 args=(3,8,17,33,2,3,0,2) + conv_mfma_bwd_weight_kernel<8,16,1,0,false> grid=(1,1,1) block=256 args=(3,8,17,33,2,3,1,2) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(8,3,8)'),
    ('bwd_weight_nhwc_cin8_cout16', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=8 Cout=16',
     'memset bytes=18432 + conv_mfma_bwd_weight_kernel<8,16,2,2,true> grid=(1,1,1) block=256 args=(8,16,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(16,8,8)'),
    ('bwd_weight_nhwc_cin8_cout32', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=8 Cout=32 W=132',
     'memset bytes=36864 + conv_mfma_bwd_weight_kernel<8,32,2,2,true> grid=(1,1,1) block=256 args=(8,32,16,132,2,9,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(32,8,8)'),
    ('bwd_weight_nhwc_cin8_nchw_dy_cout12', 'op=bwd_weight xl=2 gelu=1 dyl=1 Cin=8 Cout=12',
     'memset bytes=18432 + conv_mfma_bwd_weight_kernel<8,16,1,2,true> grid=(1,1,1) block=256 args=(8,12,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(12,8,8)'),
    ('bwd_weight_nhwc_cin8_nchw_dy_cout17', 'op=bwd_weight xl=2 gelu=1 dyl=1 Cin=8 Cout=17',
     'memset bytes=36864 + conv_mfma_bwd_weight_kernel<8,32,1,2,true> grid=(1,1,1) block=256 args=(8,17,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(17,8,8)'),
    ('bwd_weight_nhwc_cin16_cout16', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=16 Cout=16',
     'memset bytes=36864 + conv_mfma_bwd_weight_kernel<16,16,2,2,true> grid=(1,1,1) block=256 args=(16,16,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(16,16,16)'),
    ('bwd_weight_nhwc_cin16_cout32', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=16 Cout=32 B=3 H=16 W=132',
     'memset bytes=73728 + conv_mfma_bwd_weight_kernel<16,32,2,2,true> grid=(1,3,1) block=256 args=(16,32,16,132,2,9,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(32,16,16)'),
    ('bwd_weight_nhwc_cin16_nchw_dy_cout16', 'op=bwd_weight xl=2 gelu=1 dyl=1 Cin=16 Cout=16 H=1 W=1',
     'memset bytes=36864 + conv_mfma_bwd_weight_kernel<16,16,1,2,true> grid=(1,1,1) block=256 args=(16,16,1,1,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(16,16,16)'),
    ('bwd_weight_nhwc_cin16_nchw_dy_cout32', 'op=bwd_weight xl=2 gelu=1 dyl=1 Cin=16 Cout=32',
     'memset bytes=73728 + conv_mfma_bwd_weight_kernel<16,32,1,2,true> grid=(1,1,1) block=256 args=(16,32,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(32,16,16)'),
    ('bwd_weight_nhwc_cin16_det_off', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=16 Cout=32 B=3 H=17 W=33 det=0',
     'memset bytes=73728 + conv_mfma_bwd_weight_kernel<16,32,2,2,true> grid=(2,3,1) block=256 args=(16,32,17,33,2,3,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(32,16,16)'),
    ('bwd_weight_nhwc_cin16_det_on', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=16 Cout=32 B=3 H=17 W=33 det=1',
     'memset bytes=73728 + conv_mfma_bwd_weight_kernel<16,32,2,2,true> grid=(1,1,1) block=256 args=(16,32,17,33,2,3,0,0) + conv_mfma_bwd_weight_kernel<16,32,2,2,true> grid=(1,1,1) block=256 args=(16,32,17,33,2,3,1,0) + conv_mfma_bwd_weight_kernel<16,32,2,2,true> grid=(1,1,1) block=256 args=(16,32,17,33,2,3,0,1) + conv_mfma_bwd_weight_kernel<16,32,2,2,true> grid=(1,1,1) block=256 args=(16,32,17,33,2,3,1,1) + conv_mfma_bwd_weight_kernel<16,32,2,2,true> grid=(1,1,1) block=256 args=(16,32,17,33,2,3,0,2) + conv_mfma_bwd_weight_kernel<16,32,2,2,true> grid=(1,1,1) block=256 args=(16,32,17,33,2,3,1,2) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(32,16,16)'),
    ('bwd_weight_f32_dy_is_read_as_nchw', 'op=bwd_weight xl=2 gelu=1 dyl=0 Cin=8 Cout=16',
     'memset bytes=18432 + conv_mfma_bwd_weight_kernel<8,16,1,2,true> grid=(1,1,1) block=256 args=(8,16,16,16,2,1,0,0) + conv_fold_dw_kernel grid=(32,1,1) block=256 args=(16,8,8)'),
    ('bwd_weight_cin17_refused', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=17 Cout=32',
     'refused: bad args'),
    ('bwd_weight_cout33_refused', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=16 Cout=33',
     'refused: bad args'),
    ('bwd_weight_nhwc_cin12_refused', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=12 Cout=32',
     'refused: unsupported layout combination (x_layout=2 gelu=1 Cin=12)'),
    ('bwd_weight_nhwc_without_gelu_refused', 'op=bwd_weight xl=2 gelu=0 dyl=2 Cin=16 Cout=32',
     'refused: unsupported layout combination (x_layout=2 gelu=0 Cin=16)'),
    ('bwd_weight_nchw_bf16_x_refused', 'op=bwd_weight xl=1 gelu=0 dyl=2 Cin=8 Cout=16',
     'refused: unsupported layout combination (x_layout=1 gelu=0 Cin=8)'),
    ('bwd_weight_nhwc_dy_cout12_refused', 'op=bwd_weight xl=2 gelu=1 dyl=2 Cin=16 Cout=12',
     'refused: NHWC dy needs Cout % 8 == 0'),
    # ---- transpose: C == 32, W % 8, alignment; 64 | 65 pixels per row
    ('transpose_c32_w8', 'op=transpose C=32 B=2 H=3 W=8',
     'nchw_to_nhwc32_kernel grid=(1,3,2) block=256 args=(3,8)'),
    ('transpose_c32_w64', 'op=transpose C=32 B=2 H=3 W=64',
     'nchw_to_nhwc32_kernel grid=(1,3,2) block=256 args=(3,64)'),
    ('transpose_c32_w72', 'op=transpose C=32 B=2 H=3 W=72',
     'nchw_to_nhwc32_kernel grid=(2,3,2) block=256 args=(3,72)'),
    ('transpose_c32_w65', 'op=transpose C=32 B=2 H=3 W=65',
     'nchw_to_nhwc_kernel grid=(2,3,2) block=256 args=(32,3,65)'),
    ('transpose_c32_w12', 'op=transpose C=32 H=16 W=12',
     'nchw_to_nhwc_kernel grid=(1,16,1) block=256 args=(32,16,12)'),
    ('transpose_c32_misaligned', 'op=transpose C=32 B=2 H=3 W=72 aligned=0',
     'nchw_to_nhwc_kernel grid=(2,3,2) block=256 args=(32,3,72)'),
    ('transpose_c16', 'op=transpose C=16 B=2 H=3 W=64',
     'nchw_to_nhwc_kernel grid=(1,3,2) block=256 args=(16,3,64)'),
    ('transpose_c24_w132', 'op=transpose C=24 B=3 H=16 W=132',
     'nchw_to_nhwc_kernel grid=(3,16,3) block=256 args=(24,16,132)'),
    ('transpose_c33_refused', 'op=transpose C=33 H=16 W=16',
     'refused: bad args'),
    # ---- the generic path: k 3 | 4, 5 | 6, COUT_T at Cout 4 | 5, 8 | 9, 16 | 17, the four input forms, GELU' with and without the pre-activation
    ('gfwd_f32_k6_cout4', 'op=gfwd f32=1 Cin=3 Cout=4 k=6 B=2 H=17 W=33',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(4,3,6,0) + conv_direct_kernel<4,6,true,false,false> grid=(2,1,2) block=256 args=(3,4,17,33,2,1)'),
    ('gfwd_f32_k6_cout5', 'op=gfwd f32=1 Cin=3 Cout=5 k=6',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(5,3,6,0) + conv_direct_kernel<8,6,true,false,false> grid=(1,1,1) block=256 args=(3,5,16,16,2,1)'),
    ('gfwd_f32_k4_cout8', 'op=gfwd f32=1 Cin=3 Cout=8 k=4',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(8,3,4,0) + conv_direct_kernel<8,4,true,false,false> grid=(1,1,1) block=256 args=(3,8,16,16,1,1)'),
    ('gfwd_bf16_gelu_k6_cout9', 'op=gfwd f32=0 gelu=1 Cin=5 Cout=9 k=6',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(9,5,6,0) + conv_direct_kernel<16,6,false,true,false> grid=(1,1,1) block=256 args=(5,9,16,16,2,1)'),
    ('gfwd_bf16_gelu_k4_cout16', 'op=gfwd f32=0 gelu=1 Cin=5 Cout=16 k=4 W=132',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(16,5,4,0) + conv_direct_kernel<16,4,false,true,false> grid=(5,1,1) block=256 args=(5,16,16,132,1,1)'),
    ('gfwd_bf16_k6_cout17', 'op=gfwd f32=0 gelu=0 Cin=5 Cout=17 k=6 B=3',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(17,5,6,0) + conv_direct_kernel<16,6,false,false,false> grid=(1,1,6) block=256 args=(5,17,16,16,2,2)'),
    ('gfwd_bf16_k4_cout33', 'op=gfwd f32=0 gelu=0 Cin=33 Cout=33 k=4 B=3 H=17 W=33',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(33,33,4,0) + conv_direct_kernel<16,4,false,false,false> grid=(2,1,9) block=256 args=(33,33,17,33,1,3)'),
    ('gfwd_f32_gelu_k6', 'op=gfwd f32=1 gelu=1 Cin=5 Cout=24 k=6',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(24,5,6,0) + conv_direct_kernel<16,6,true,true,false> grid=(1,1,2) block=256 args=(5,24,16,16,2,2)'),
    ('gfwd_f32_gelu_k4', 'op=gfwd f32=1 gelu=1 Cin=5 Cout=3 k=4 H=1 W=1',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(3,5,4,0) + conv_direct_kernel<4,4,true,true,false> grid=(1,1,1) block=256 args=(5,3,1,1,1,1)'),
    ('gfwd_k3_refused', 'op=gfwd f32=1 Cin=3 Cout=16 k=3',
     'refused: kernel size 3 unsupported (4 or 6)'),
    ('gfwd_k5_refused', 'op=gfwd f32=1 Cin=3 Cout=16 k=5',
     'refused: kernel size 5 unsupported (4 or 6)'),
    ('gfwd_null_pointer_refused', 'op=gfwd f32=1 Cin=3 Cout=16 ptr=0',
     'refused: bad args'),
    ('gbwd_data_dgelu_k6_cin3', 'op=gbwd_data gelu=1 Cin=3 Cout=6 k=6 B=2 H=17 W=33',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(6,3,6,1) + conv_direct_kernel<4,6,false,false,true> grid=(2,1,2) block=256 args=(6,3,17,33,3,1)'),
    ('gbwd_data_dgelu_k4_cin8', 'op=gbwd_data gelu=1 Cin=8 Cout=6 k=4',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(6,8,4,1) + conv_direct_kernel<8,4,false,false,true> grid=(1,1,1) block=256 args=(6,8,16,16,2,1)'),
    ('gbwd_data_dgelu_k6_cin16', 'op=gbwd_data gelu=1 Cin=16 Cout=6 k=6',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(6,16,6,1) + conv_direct_kernel<16,6,false,false,true> grid=(1,1,1) block=256 args=(6,16,16,16,3,1)'),
    ('gbwd_data_plain_k6_cin16', 'op=gbwd_data gelu=0 Cin=16 Cout=6 k=6',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(6,16,6,1) + conv_direct_kernel<16,6,false,false,false> grid=(1,1,1) block=256 args=(6,16,16,16,3,1)'),
    ('gbwd_data_plain_without_pre_k4_cin17', 'op=gbwd_data gelu=0 pre=0 Cin=17 Cout=6 k=4',
     'repack_weights_kernel grid=(32,1,1) block=256 args=(6,17,4,1) + conv_direct_kernel<16,4,false,false,false> grid=(1,1,2) block=256 args=(6,17,16,16,2,2)'),
    ('gbwd_data_dgelu_without_pre_refused', 'op=gbwd_data gelu=1 pre=0 Cin=3 Cout=16 k=6',
     'refused: in_gelu needs the stored pre-activation'),
    ('gbwd_data_k3_refused', 'op=gbwd_data gelu=0 pre=0 Cin=3 Cout=16 k=3',
     'refused: kernel size 3 unsupported (4 or 6)'),
    ('gbwd_weight_f32_k6_cout4', 'op=gbwd_weight f32=1 Cin=5 Cout=4 k=6',
     'conv_bwd_weight_kernel<4,6,true,false> grid=(1,1,1) block=256 args=(5,16,16,2,0,0,0)'),
    ('gbwd_weight_f32_k4_cout8', 'op=gbwd_weight f32=1 Cin=5 Cout=8 k=4 B=3 H=17 W=33',
     'conv_bwd_weight_kernel<8,4,true,false> grid=(2,1,3) block=256 args=(5,17,33,1,0,0,0)'),
    ('gbwd_weight_bf16_gelu_k6_cout16', 'op=gbwd_weight f32=0 gelu=1 Cin=5 Cout=16 k=6 W=132',
     'conv_bwd_weight_kernel<16,6,false,true> grid=(5,1,1) block=256 args=(5,16,132,2,0,0,0)'),
    ('gbwd_weight_bf16_gelu_k4_cout32', 'op=gbwd_weight f32=0 gelu=1 Cin=5 Cout=32 k=4',
     'conv_bwd_weight_kernel<32,4,false,true> grid=(1,1,1) block=256 args=(5,16,16,1,0,0,0)'),
    ('gbwd_weight_bf16_k6_cout32', 'op=gbwd_weight f32=0 gelu=0 Cin=5 Cout=32 k=6',
     'conv_bwd_weight_kernel<32,6,false,false> grid=(1,1,1) block=256 args=(5,16,16,2,0,0,0)'),
    ('gbwd_weight_bf16_k4_cout4', 'op=gbwd_weight f32=0 gelu=0 Cin=5 Cout=4 k=4',
     'conv_bwd_weight_kernel<4,4,false,false> grid=(1,1,1) block=256 args=(5,16,16,1,0,0,0)'),
    ('gbwd_weight_bf16_k6_cout8', 'op=gbwd_weight f32=0 gelu=0 Cin=5 Cout=8 k=6',
     'conv_bwd_weight_kernel<8,6,false,false> grid=(1,1,1) block=256 args=(5,16,16,2,0,0,0)'),
    ('gbwd_weight_bf16_gelu_k4_cout16', 'op=gbwd_weight f32=0 gelu=1 Cin=5 Cout=16 k=4',
     'conv_bwd_weight_kernel<16,4,false,true> grid=(1,1,1) block=256 args=(5,16,16,1,0,0,0)'),
    ('gbwd_weight_det_off', 'op=gbwd_weight f32=1 Cin=3 Cout=16 k=6 B=2 H=17 W=33 det=0',
     'conv_bwd_weight_kernel<16,6,true,false> grid=(2,1,2) block=256 args=(3,17,33,2,0,0,0)'),
    ('gbwd_weight_det_on', 'op=gbwd_weight f32=1 Cin=3 Cout=16 k=6 B=2 H=17 W=33 det=1',
     'conv_bwd_weight_kernel<16,6,true,false> grid=(1,1,1) block=256 args=(3,17,33,2,0,0,0) + conv_bwd_weight_kernel<16,6,true,false> grid=(1,1,1) block=256 args=(3,17,33,2,1,0,0) + conv_bwd_weight_kernel<16,6,true,false> grid=(1,1,1) block=256 args=(3,17,33,2,0,0,1) + conv_bwd_weight_kernel<16,6,true,false> grid=(1,1,1) block=256 args=(3,17,33,2,1,0,1)'),
    ('gbwd_weight_cout12_refused', 'op=gbwd_weight f32=1 Cin=3 Cout=12 k=6',
     'refused: Cout=12 k=6 unsupported (Cout in {4,8,16,32}, k in {4,6})'),
    ('gbwd_weight_cout33_refused', 'op=gbwd_weight f32=1 Cin=3 Cout=33 k=6',
     'refused: Cout=33 k=6 unsupported (Cout in {4,8,16,32}, k in {4,6})'),
    ('gbwd_weight_k5_refused', 'op=gbwd_weight f32=1 Cin=3 Cout=16 k=5',
     'refused: Cout=16 k=5 unsupported (Cout in {4,8,16,32}, k in {4,6})'),
    ('gbwd_weight_f32_gelu_refused', 'op=gbwd_weight f32=1 gelu=1 Cin=3 Cout=16 k=6',
     'refused: f32+gelu input combination unsupported'),
]

# not recorded: the parent's host code let these through to a launch with an empty grid (or read channel -4 of the pre-activation)
NOW_REFUSED = [(f'{op}_{field}0', f'op={op} {more} {field}=0') for op, more in
               (('fwd', 'xl=0 Cin=3 Cout=16 nchw=1'), ('bwd_data', 'dyl=2 Cin=16 Cout=32'), ('bwd_weight', 'xl=2 gelu=1 dyl=2 Cin=16 Cout=32'), ('transpose', 'C=32'),
                ('gfwd', 'f32=1 Cin=3 Cout=16'), ('gbwd_data', 'Cin=3 Cout=16'), ('gbwd_weight', 'f32=1 Cin=3 Cout=16'))
               for field in ('H', 'W', 'B') + (('C',) if op == 'transpose' else ('Cin', 'Cout'))]


@pytest.fixture(scope='module')
def route_cli(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler found (set CXX)'
    exe = str(tmp_path_factory.mktemp('conv_route') / 'conv_route_cli')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', os.path.join(ROOT, 'tests', 'conv_route_cli.cpp'), '-o', exe],
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


def test_empty_problems_are_refused_by_the_one_check(route_cli):
    got = routes(route_cli, NOW_REFUSED)
    assert len(got) == len(NOW_REFUSED) == 7 * 5 - 1
    assert set(got.values()) == {'refused: bad args'}, {n: r for n, r in got.items() if r != 'refused: bad args'}


def kernels_of(route):
    return re.findall(r'(\w+_kernel(?:<[^>]*>)?) grid', route)


def test_the_table_covers_every_route_kind_and_knob(route_cli):
    names = [name for name, _, _ in TABLE]
    assert len(set(names)) == len(names)
    launched = {k for _, _, route in TABLE for k in kernels_of(route)}
    # every instantiation of the MFMA path, and of the generic path every COUT_T / COUT, k and input form
    for t in instantiated(route_cli):
        if t.startswith(('conv_mfma', 'nchw_to')):
            assert numeric(t) in launched, t
    for k in (f'conv_direct_kernel<{t},{k},' for t in (4, 8, 16) for k in (4, 6)):
        assert any(x.startswith(k) for x in launched), k
    for form in ('true,false,false', 'false,true,false', 'false,false,false', 'true,true,false', 'false,false,true'):
        assert any(x.startswith('conv_direct_kernel<') and x.endswith(form + '>') for x in launched), form
    for k in (f'conv_bwd_weight_kernel<{t},{k},' for t in (4, 8, 16, 32) for k in (4, 6)):
        assert any(x.startswith(k) for x in launched), k
    for form in ('true,false', 'false,true', 'false,false'):
        assert any(x.startswith('conv_bwd_weight_kernel<') and x.endswith(',' + form + '>') for x in launched), form
    for k in ('conv_repack_kernel', 'conv_fold_dw_kernel', 'repack_weights_kernel'):
        assert k in launched, k
    # every refusal message
    text = '\n'.join(route for _, _, route in TABLE)
    for why in ('bad args', 'NHWC input needs 8/16/32 channels', 'NHWC output needs Cout % 8 == 0', 'unsupported layout combination (src=', 'dy layout',
                'NHWC dy needs Cout % 8 == 0', 'unsupported layout combination (x_layout=', 'kernel size 3 unsupported (4 or 6)', 'kernel size 5 unsupported (4 or 6)',
                'in_gelu needs the stored pre-activation', 'f32+gelu input combination unsupported', 'Cout=12 k=6 unsupported (Cout in {4,8,16,32}, k in {4,6})',
                'Cout=16 k=5 unsupported'):
        assert 'refused: ' + why in text, why
    for op in ('fwd', 'bwd_data', 'bwd_weight', 'transpose', 'gfwd'):
        assert any(f'op={op} ' in call and route == 'refused: bad args' for _, call, route in TABLE), op
    # both sides of every boundary of the rule
    field = lambda call, key, dflt: int((re.search(rf'\b{key}=(\d+)', call) or [0, dflt])[1])
    seen = {(re.search(r'op=(\w+)', call)[1], key, field(call, key, None), field(call, 'xl', 2) if key == 'Cin' else 2)
            for _, call, _ in TABLE for key in ('Cin', 'Cout') if re.search(rf'\b{key}=', call)}
    for op, key, values in (('fwd', 'Cin', (8, 9, 16, 17, 32, 33)), ('fwd', 'Cout', (16, 17, 32, 33)), ('bwd_data', 'Cout', (8, 9, 16, 17, 32, 33)),
                            ('bwd_data', 'Cin', (8, 16, 17)), ('bwd_weight', 'Cin', (8, 9, 16, 17)), ('bwd_weight', 'Cout', (16, 17, 32, 33)),
                            ('gfwd', 'Cout', (4, 5, 8, 9, 16, 17)), ('gbwd_data', 'Cin', (3, 8, 16, 17)), ('gbwd_weight', 'Cout', (4, 8, 16, 32, 33))):
        for v in values:
            assert any(o == op and k == key and x == v for o, k, x, _ in seen), (op, key, v)
    for op in ('fwd', 'bwd_weight'):                        # the image: 4 | 5 channels (the staging sub-route inside the kernel), 8 | 9
        for v in (4, 5, 8, 9):
            assert (op, 'Cin', v, 0) in seen, (op, 'image Cin', v)
    nhwc_io = {field(call, 'Cout', 16) % 8 == 0 for _, call, _ in TABLE if 'op=fwd xl=2' in call and 'nchw=1' not in call}
    assert nhwc_io == {False, True}
    tr = [(field(call, 'C', 32), field(call, 'W', 16), field(call, 'aligned', 1), route) for _, call, route in TABLE if 'op=transpose' in call]
    assert {(c == 32, w % 8 == 0, bool(a)) for c, w, a, _ in tr} >= {(True, True, True), (True, False, True), (True, True, False), (False, True, True)}
    assert {w for _, w, _, _ in tr} >= {64, 65}
    for op in ('fwd', 'bwd_data', 'bwd_weight'):            # tiles_x = 1 and 9 (the last argument of the conv kernel before by, bz)
        ws = {field(call, 'W', 16) for _, call, route in TABLE if f'op={op} ' in call and not route.startswith('refused')}
        assert {(w + 15) // 16 for w in ws} >= {1, 9}, (op, ws)
    for op in ('bwd_weight', 'gbwd_weight'):
        assert {field(call, 'det', 0) for _, call, route in TABLE if f'op={op} ' in call and not route.startswith('refused')} == {0, 1}, op
        serial = [route for _, call, route in TABLE if f'op={op} ' in call and 'det=1' in call]
        assert serial and all(route.count('bwd_weight_kernel<') > 1 and 'grid=(1,1,1)' in route for route in serial)


# ---------------------------------------------------------------------------------------------- conv_ref.route against the header
SRC = {'0': 'SRC_NCHW_F32', '1': 'SRC_NCHW_BF16', '2': 'SRC_NHWC_BF16'}
LAYOUT = {'img': 0, 'nchw': 1, 'nhwc': 2}


def spelled(kernel):
    """'conv_mfma_kernel<8,1,0,false,false,false,4,1>' in the words of conv_ref.route (NW and GRP follow from the others: left out)"""
    name, targs = re.fullmatch(r'(\w+)<([^>]*)>', kernel).groups()
    a = targs.split(',')
    if name == 'conv_mfma_kernel':
        return f'{name}<{a[0]}, {a[1]}, {SRC[a[2]]}, {a[3]}, {a[4]}, {a[5]}>'
    assert name == 'conv_mfma_bwd_weight_kernel', kernel
    return f'{name}<{a[0]}, {a[1]}, {SRC[a[2]]}, {SRC[a[3]]}, {a[4]}>'


def numeric(kernel):
    """the inverse of spelled(), for a member of the instantiated set: with NW and GRP as csrc/conv_route.h::conv6_targs derives them"""
    if '<' not in kernel:
        return kernel
    name, targs = re.fullmatch(r'(\w+)<([^>]*)>', kernel).groups()
    a = [{v: k for k, v in SRC.items()}.get(x, x) for x in targs.split(', ')]
    if name == 'conv_mfma_kernel':
        cp, nchw = int(a[0]), a[5] == 'true'
        a += [str(8 if cp == 32 or (nchw and cp == 16) else 4), str(R.GRP if nchw and cp >= 16 else 1)]
    return f'{name}<{",".join(a)}>'


def instantiated(exe):
    """{kernel as conv_ref spells it: its workspace need} of the CLI's --set listing"""
    r = subprocess.run([exe, '--set'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        kernel, _, rest = line.partition('> ')
        out[kernel + ('>' if '<' in line else '')] = dict(kv.split('=') for kv in rest.split()) if rest else {}
    return out


def call_of(c, det=0):
    if c.op == 'fwd':
        return f"op=fwd xl={LAYOUT[c.src]} gelu={int(c.src == 'nhwc')} nchw={int(c.dst == 'nchw')} B={c.B} Cin={c.Cin} Cout={c.Cout} H={c.H} W={c.W}"
    if c.op == 'bwd_data':
        return f'op=bwd_data dyl={LAYOUT[c.dyl]} B={c.B} Cin={c.Cin} Cout={c.Cout} H={c.H} W={c.W}'
    return f"op=bwd_weight xl={LAYOUT[c.src]} gelu={int(c.src == 'nhwc')} dyl={LAYOUT[c.dyl]} B={c.B} Cin={c.Cin} Cout={c.Cout} H={c.H} W={c.W} det={det}"


def test_the_python_restatement_agrees_with_the_header(route_cli):
    cases = [(c, 0) for c in R.FWD_CASES + R.BWD_DATA_CASES + R.BWD_WEIGHT_CASES] + [(c, 1) for c in R.DET_CASES]
    assert len(cases) > 100
    got = routes(route_cli, [(str(i), call_of(c, det)) for i, (c, det) in enumerate(cases)])
    for i, (c, det) in enumerate(cases):
        conv = [k for k in kernels_of(got[str(i)]) if k.startswith('conv_mfma')]
        assert len(set(conv)) == 1 and len(conv) == (((c.H + 15) // 16) * c.B if det else 1), (c.id, got[str(i)])
        assert spelled(conv[0]) == re.sub(r'/(chunks|planar)$', '', R.route(c)), (c.id, got[str(i)], R.route(c))
    got = routes(route_cli, [(f'{C},{W},{mis}', f'op=transpose C={C} W={W} B=2 H=3 aligned={int(not mis)}') for C, W, mis in R.T_CASES])
    for C, W, mis in R.T_CASES:
        assert kernels_of(got[f'{C},{W},{mis}']) == [R.transpose_route(C, W, not mis)], (C, W, mis)


def test_the_instantiated_set_is_all_routes(route_cli):
    inst = instantiated(route_cli)
    mfma = {k for k in inst if k.startswith(('conv_mfma', 'nchw_to'))}
    assert mfma == {re.sub(r'/(chunks|planar)$', '', r) for r in R.all_routes()}, sorted(mfma ^ {re.sub(r'/(chunks|planar)$', '', r) for r in R.all_routes()})
    assert len(mfma) == 22 + 12 + 2
    # the generic path: COUT_T x k x (four forward input forms + GELU' on bf16); COUT x k x (every input form but fp32 + GELU)
    assert sum(k.startswith('conv_direct_kernel<') for k in inst) == 3 * 2 * 5 and sum(k.startswith('conv_bwd_weight_kernel<') for k in inst) == 4 * 2 * 3
    # every accepted row of the table launches members only
    for _, call, route in TABLE:
        for k in kernels_of(route):
            if k.startswith('conv_mfma'):
                assert spelled(k) in inst and numeric(spelled(k)) == k, (call, k)


# -------------------------------------------------------------------------------- ops.conv_stack_takes_mfma against the routes
WIDTHS = (1, 3, 4, 5, 8, 12, 16, 24, 32, 33)
ONLY_THE_ROUTE = set()          # stacks (k = 6) every call of which the header accepts although the engine keeps them on the generic path: none


def stack_calls(chans):
    """the calls encode / encode_backward make for a stack on the MFMA path (engine.py), as CLI calls"""
    n, calls = len(chans) - 1, []
    # the projector's gradient is transposed once where every kernel that reads it takes it NHWC: a multiple of 8 channels for the
    # weight gradient, 8 / 16 / 32 for the data gradient of a deeper stack.  (Until this test existed the engine transposed every
    # multiple of 8: a stack of two or more layers ending in 24 channels was refused by i2t_conv6_bwd_data, 'dy layout'.)
    last_nhwc = chans[-1] % 8 == 0 and (n == 1 or chans[-1] in (8, 16, 32))
    if last_nhwc:
        calls.append(f'op=transpose C={chans[-1]}')
    for i in range(n):
        cin, cout, last = chans[i], chans[i + 1], i == n - 1
        x = f'xl={0 if i == 0 else 2} gelu={int(i > 0)}'
        dyl = 2 if (not last or last_nhwc) else 1
        calls.append(f'op=fwd {x} nchw={int(last)} Cin={cin} Cout={cout}')
        calls.append(f'op=bwd_weight {x} dyl={dyl} Cin={cin} Cout={cout}')
        if i > 0:
            calls.append(f'op=bwd_data dyl={dyl} Cin={cin} Cout={cout}')
    return calls


def test_the_engine_takes_the_mfma_path_only_where_every_call_is_accepted(route_cli):
    from image2text_amd import ops
    stacks = [ch for n in (1, 2, 3, 4) for ch in itertools.product(WIDTHS, repeat=n + 1)]
    assert len(stacks) == 10 ** 2 + 10 ** 3 + 10 ** 4 + 10 ** 5
    calls = {ch: stack_calls(ch) for ch in stacks}
    distinct = sorted({c for cs in calls.values() for c in cs})
    got = routes(route_cli, [(str(i), c + ' B=3 H=17 W=33') for i, c in enumerate(distinct)])
    accepted = {c: not got[str(i)].startswith('refused') for i, c in enumerate(distinct)}
    assert any(accepted.values()) and not all(accepted.values())
    only_route = set()
    for ch in stacks:
        ok = all(accepted[c] for c in calls[ch])
        assert not ops.conv_stack_takes_mfma(list(ch), 4)                       # the MFMA kernels are 6x6
        if ops.conv_stack_takes_mfma(list(ch), 6):
            assert ok, (ch, [c for c in calls[ch] if not accepted[c]])
        elif ok:
            only_route.add(ch)
    assert sum(ops.conv_stack_takes_mfma(list(ch), 6) for ch in stacks) > 100
    assert only_route == ONLY_THE_ROUTE, sorted(only_route ^ ONLY_THE_ROUTE)[:10]


def test_the_workspaces_cover_every_instantiation(route_cli):
    from image2text_amd import ops
    inst = instantiated(route_cli)
    ws = [int(v['ws_elems']) for v in inst.values() if 'ws_elems' in v]
    scratch = [int(v['scratch_floats']) for v in inst.values() if 'scratch_floats' in v]
    assert len(ws) == 22 and len(scratch) == 12
    assert ops.CONV6_WS_ELEMS >= max(ws) and ops.CONV6_SCRATCH_FLOATS >= max(scratch), (max(ws), max(scratch))
    # and the routes ask for what the listing says: the largest of each in the table
    rows = dict((name, route) for name, _, route in TABLE)
    assert 'args=(32,32,32,32,0)' in rows['fwd_nhwc_cin32_cout32'] and 32 * 36 * 32 == max(ws)               # rows_p, red_p of the repack
    assert f'memset bytes={4 * max(scratch)} ' in rows['bwd_weight_nhwc_cin16_cout32']
