"""The GEMM host layer's plans (csrc/gemm_plan.hip), read through mmg_gemm_plan: no GPU, nothing is launched.

What a plan string holds: the kernel instantiation as mmg_last_kernel() spells it, " grid=(x,y) block=T lds=B", and for the weight-gradient
ops " chunks=.. rows=.. xcd=.. swapped=.." (+ " split=.." for the 8-bit ones).  Every plan is made for 256 CUs (the MI355X)."""
import re

import pytest

from mmgclip import _hip

CUS = 256
DOORS = {0: "mmg_gemm_nt_bf16", 1: "mmg_gemm_nt_fp8", 2: "mmg_gemm_nt_fp8_bwd", 3: "mmg_gemm_nt_fp8_bwd", 4: "mmg_gemm_tn_bf16",
         5: "mmg_gemm_tn_fp8", 6: "mmg_gemm_tn_fp8"}

# (op, M, N, K) -> plan under default knobs.  The shapes: those of test_gemm_gpu.py::test_launched_kernel_is_the_planned_one, then the towers of
# bench.py - ConvNeXt-T / -B blocks and 2 x 2 downsampling layers per stage (pixel rows of 64 images of 224 x 224), the 8-bit path of ConvNeXt-B,
# BERT (128 x 77 tokens) and ViT-B/16 (64 x 197 tokens) with 768 / 2304 / 3072, the projection heads (128 rows).
SELECTION = {
    (0, 256, 128, 64): 'gemm_nt_kernel<128, 128, 32, 2, 3, 0> grid=(2,1) block=256 lds=49152',
    (0, 300, 200, 160): 'gemm_nt_kernel<128, 128, 32, 2, 2, 0> grid=(6,1) block=256 lds=33792',
    (0, 64, 512, 768): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(4,1) block=256 lds=65536',
    (0, 256, 96, 96): 'gemm_nt_kernel<128, 96, 32, 2, 2, 0> grid=(2,1) block=256 lds=28672',
    (0, 256, 96, 128): 'gemm_nt_kernel<128, 96, 64, 2, 2, 0> grid=(2,1) block=256 lds=57344',
    (0, 16424, 512, 384): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(130,1) block=512 lds=131072',
    (0, 21800, 384, 384): 'gemm_nt_kernel<256, 192, 64, 4, 2, 0> grid=(172,1) block=512 lds=114688',
    (0, 4100, 128, 4096): 'gemm_nt_kernel<256, 128, 64, 4, 3, 0> grid=(17,1) block=512 lds=147456',
    (1, 256, 256, 128): 'gemm_nt_kernel<128, 128, 64, 2, 2, 1> grid=(4,1) block=256 lds=65536',
    (1, 4096, 256, 512): 'gemm_nt_kernel<256, 256, 64, 4, 2, 1> grid=(16,1) block=512 lds=131072',
    (1, 4100, 384, 256): 'gemm_nt_kernel<256, 128, 64, 4, 3, 1> grid=(51,1) block=512 lds=147456',
    (2, 640, 384, 128): 'gemm_nt_kernel<128, 128, 64, 2, 2, 2> grid=(15,1) block=256 lds=65536',
    (3, 640, 384, 128): 'gemm_nt_kernel<128, 128, 64, 2, 2, 1> grid=(15,1) block=256 lds=65536',
    (2, 4096, 256, 128): 'gemm_nt_kernel<256, 256, 64, 4, 2, 2> grid=(16,1) block=512 lds=131072',
    (3, 4096, 256, 128): 'gemm_nt_kernel<256, 256, 64, 4, 2, 1> grid=(16,1) block=512 lds=131072',
    (4, 256, 128, 128): 'gemm_tn_kernel<1, 1, 64> grid=(8,1) block=256 lds=65536 chunks=4 rows=64 xcd=1 swapped=0',
    (4, 32768, 128, 256): 'gemm_tn_kernel<1, 2, 32> grid=(512,1) block=256 lds=66560 chunks=512 rows=64 xcd=1 swapped=0',
    (4, 32768, 256, 128): 'gemm_tn_kernel<2, 1, 32> grid=(512,1) block=256 lds=49152 chunks=512 rows=64 xcd=2 swapped=0',
    (4, 65536, 192, 384): 'gemm_tn_wide_kernel<192, 384> grid=(256,1) block=512 lds=148992 chunks=256 rows=256 xcd=0 swapped=0',
    (4, 65536, 384, 192): 'gemm_tn_wide_kernel<192, 384> grid=(256,1) block=512 lds=148992 chunks=256 rows=256 xcd=0 swapped=1',
    (4, 65536, 96, 384): 'gemm_tn_wide_kernel<96, 384> grid=(256,1) block=512 lds=148992 chunks=256 rows=256 xcd=0 swapped=0',
    (4, 65536, 128, 512): 'gemm_tn_wide_kernel<128, 256> grid=(256,1) block=512 lds=98304 chunks=128 rows=512 xcd=0 swapped=0',
    (4, 65536, 256, 1024): 'gemm_tn_wide_kernel<256, 256> grid=(256,1) block=512 lds=133120 chunks=64 rows=1024 xcd=0 swapped=0',
    (4, 65599, 200, 392): 'gemm_tn_kernel<1, 1, 64> grid=(496,1) block=256 lds=65536 chunks=61 rows=1088 xcd=1 swapped=0',
    (5, 384, 128, 256): 'gemm_tn8_kernel<1> grid=(8,1) block=256 lds=65536 chunks=3 rows=128 xcd=1 swapped=0 split=2',
    (6, 384, 128, 256): 'gemm_tn8_kernel<0> grid=(8,1) block=256 lds=65536 chunks=3 rows=128 xcd=1 swapped=0 split=2',
    (5, 8192, 256, 256): 'gemm_tn8_wide_kernel<1> grid=(64,1) block=512 lds=131072 chunks=64 rows=128 xcd=1 swapped=0 split=1',
    (6, 8192, 256, 256): 'gemm_tn8_wide_kernel<0> grid=(64,1) block=512 lds=131072 chunks=64 rows=128 xcd=1 swapped=0 split=1',
    (5, 8191, 256, 256): 'gemm_tn8_kernel<1> grid=(256,1) block=256 lds=65536 chunks=64 rows=128 xcd=1 swapped=0 split=1',
    (6, 8191, 256, 256): 'gemm_tn8_kernel<0> grid=(256,1) block=256 lds=65536 chunks=64 rows=128 xcd=1 swapped=0 split=1',
    (0, 200704, 384, 96): 'gemm_nt_kernel<128, 128, 32, 2, 3, 0> grid=(4704,1) block=256 lds=49152',
    (0, 200704, 96, 384): 'gemm_nt_kernel<128, 96, 64, 2, 2, 0> grid=(1568,1) block=256 lds=57344',
    (4, 200704, 384, 96): 'gemm_tn_wide_kernel<96, 384> grid=(256,1) block=512 lds=148992 chunks=256 rows=800 xcd=0 swapped=1',
    (4, 200704, 96, 384): 'gemm_tn_wide_kernel<96, 384> grid=(256,1) block=512 lds=148992 chunks=256 rows=800 xcd=0 swapped=0',
    (0, 50176, 768, 192): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(2352,1) block=256 lds=65536',
    (0, 50176, 192, 768): 'gemm_nt_kernel<256, 192, 64, 4, 2, 0> grid=(196,1) block=512 lds=114688',
    (4, 50176, 768, 192): 'gemm_tn_kernel<2, 1, 32> grid=(480,1) block=256 lds=49152 chunks=79 rows=640 xcd=2 swapped=0',
    (4, 50176, 192, 768): 'gemm_tn_kernel<1, 2, 32> grid=(480,1) block=256 lds=66560 chunks=79 rows=640 xcd=1 swapped=0',
    (0, 12544, 1536, 384): 'gemm_nt_kernel<256, 192, 64, 4, 2, 0> grid=(392,1) block=512 lds=114688',
    (0, 12544, 384, 1536): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(294,1) block=256 lds=65536',
    (4, 12544, 1536, 384): 'gemm_tn_kernel<1, 1, 64> grid=(504,1) block=256 lds=65536 chunks=14 rows=896 xcd=2 swapped=0',
    (4, 12544, 384, 1536): 'gemm_tn_kernel<1, 1, 64> grid=(504,1) block=256 lds=65536 chunks=14 rows=896 xcd=1 swapped=0',
    (0, 3136, 3072, 768): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(600,1) block=256 lds=65536',
    (0, 3136, 768, 3072): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(150,1) block=256 lds=65536',
    (4, 3136, 3072, 768): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=3 rows=1088 xcd=2 swapped=0',
    (4, 3136, 768, 3072): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=3 rows=1088 xcd=1 swapped=0',
    (0, 50176, 192, 384): 'gemm_nt_kernel<256, 192, 64, 4, 2, 0> grid=(196,1) block=512 lds=114688',
    (0, 50176, 384, 192): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(1176,1) block=256 lds=65536',
    (4, 50176, 384, 192): 'gemm_tn_kernel<1, 1, 64> grid=(480,1) block=256 lds=65536 chunks=79 rows=640 xcd=2 swapped=0',
    (0, 12544, 384, 768): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(294,1) block=256 lds=65536',
    (0, 12544, 768, 384): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(147,1) block=512 lds=131072',
    (4, 12544, 768, 384): 'gemm_tn_kernel<1, 1, 64> grid=(504,1) block=256 lds=65536 chunks=28 rows=448 xcd=2 swapped=0',
    (0, 3136, 768, 1536): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(150,1) block=256 lds=65536',
    (0, 3136, 1536, 768): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(300,1) block=256 lds=65536',
    (4, 3136, 1536, 768): 'gemm_tn_kernel<1, 1, 64> grid=(72,7) block=256 lds=65536 chunks=7 rows=448 xcd=0 swapped=0',
    (0, 200704, 512, 128): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(6272,1) block=256 lds=65536',
    (0, 200704, 128, 512): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(1568,1) block=256 lds=65536',
    (4, 200704, 512, 128): 'gemm_tn_wide_kernel<128, 256> grid=(256,1) block=512 lds=98304 chunks=128 rows=1568 xcd=0 swapped=1',
    (4, 200704, 128, 512): 'gemm_tn_wide_kernel<128, 256> grid=(256,1) block=512 lds=98304 chunks=128 rows=1568 xcd=0 swapped=0',
    (0, 50176, 1024, 256): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(3136,1) block=256 lds=65536',
    (0, 50176, 256, 1024): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(196,1) block=512 lds=131072',
    (4, 50176, 1024, 256): 'gemm_tn_kernel<2, 1, 32> grid=(496,1) block=256 lds=49152 chunks=61 rows=832 xcd=2 swapped=0',
    (4, 50176, 256, 1024): 'gemm_tn_kernel<1, 2, 32> grid=(496,1) block=256 lds=66560 chunks=61 rows=832 xcd=1 swapped=0',
    (0, 12544, 2048, 512): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(392,1) block=512 lds=131072',
    (0, 12544, 512, 2048): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(392,1) block=256 lds=65536',
    (4, 12544, 2048, 512): 'gemm_tn_kernel<1, 1, 64> grid=(512,1) block=256 lds=65536 chunks=8 rows=1600 xcd=2 swapped=0',
    (4, 12544, 512, 2048): 'gemm_tn_kernel<1, 1, 64> grid=(512,1) block=256 lds=65536 chunks=8 rows=1600 xcd=1 swapped=0',
    (0, 3136, 4096, 1024): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(800,1) block=256 lds=65536',
    (0, 3136, 1024, 4096): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(200,1) block=256 lds=65536',
    (4, 3136, 4096, 1024): 'gemm_tn_kernel<1, 1, 64> grid=(512,1) block=256 lds=65536 chunks=2 rows=1600 xcd=2 swapped=0',
    (4, 3136, 1024, 4096): 'gemm_tn_kernel<1, 1, 64> grid=(512,1) block=256 lds=65536 chunks=2 rows=1600 xcd=1 swapped=0',
    (0, 50176, 256, 512): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(196,1) block=512 lds=131072',
    (0, 50176, 512, 256): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(1568,1) block=256 lds=65536',
    (4, 50176, 512, 256): 'gemm_tn_kernel<2, 1, 32> grid=(448,1) block=256 lds=49152 chunks=112 rows=448 xcd=2 swapped=0',
    (0, 12544, 512, 1024): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(392,1) block=256 lds=65536',
    (0, 12544, 1024, 512): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(196,1) block=512 lds=131072',
    (4, 12544, 1024, 512): 'gemm_tn_kernel<1, 1, 64> grid=(512,1) block=256 lds=65536 chunks=16 rows=832 xcd=2 swapped=0',
    (0, 3136, 1024, 2048): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(200,1) block=256 lds=65536',
    (0, 3136, 2048, 1024): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(400,1) block=256 lds=65536',
    (4, 3136, 2048, 1024): 'gemm_tn_kernel<1, 1, 64> grid=(512,1) block=256 lds=65536 chunks=4 rows=832 xcd=2 swapped=0',
    (1, 50176, 1024, 256): 'gemm_nt_kernel<256, 256, 64, 4, 2, 1> grid=(784,1) block=512 lds=131072',
    (1, 50176, 256, 1024): 'gemm_nt_kernel<256, 256, 64, 4, 2, 1> grid=(196,1) block=512 lds=131072',
    (2, 50176, 1024, 256): 'gemm_nt_kernel<256, 256, 64, 4, 2, 2> grid=(784,1) block=512 lds=131072',
    (2, 50176, 256, 1024): 'gemm_nt_kernel<256, 256, 64, 4, 2, 2> grid=(196,1) block=512 lds=131072',
    (5, 50176, 1024, 256): 'gemm_tn8_wide_kernel<1> grid=(224,1) block=512 lds=131072 chunks=56 rows=896 xcd=1 swapped=0 split=1',
    (5, 50176, 256, 1024): 'gemm_tn8_wide_kernel<1> grid=(224,1) block=512 lds=131072 chunks=56 rows=896 xcd=1 swapped=0 split=1',
    (1, 12544, 2048, 512): 'gemm_nt_kernel<256, 256, 64, 4, 2, 1> grid=(392,1) block=512 lds=131072',
    (1, 12544, 512, 2048): 'gemm_nt_kernel<256, 256, 64, 4, 2, 1> grid=(98,1) block=512 lds=131072',
    (2, 12544, 2048, 512): 'gemm_nt_kernel<256, 256, 64, 4, 2, 2> grid=(392,1) block=512 lds=131072',
    (2, 12544, 512, 2048): 'gemm_nt_kernel<256, 256, 64, 4, 2, 2> grid=(98,1) block=512 lds=131072',
    (5, 12544, 2048, 512): 'gemm_tn8_wide_kernel<1> grid=(224,1) block=512 lds=131072 chunks=14 rows=896 xcd=1 swapped=0 split=4',
    (5, 12544, 512, 2048): 'gemm_tn8_wide_kernel<1> grid=(224,1) block=512 lds=131072 chunks=14 rows=896 xcd=1 swapped=0 split=4',
    (1, 3136, 4096, 1024): 'gemm_nt_kernel<128, 128, 64, 2, 2, 1> grid=(800,1) block=256 lds=65536',
    (1, 3136, 1024, 4096): 'gemm_nt_kernel<128, 128, 64, 2, 2, 1> grid=(200,1) block=256 lds=65536',
    (2, 3136, 4096, 1024): 'gemm_nt_kernel<128, 128, 64, 2, 2, 2> grid=(800,1) block=256 lds=65536',
    (2, 3136, 1024, 4096): 'gemm_nt_kernel<128, 128, 64, 2, 2, 2> grid=(200,1) block=256 lds=65536',
    (5, 3136, 4096, 1024): 'gemm_tn8_kernel<1> grid=(1024,1) block=256 lds=65536 chunks=4 rows=896 xcd=1 swapped=0 split=2',
    (5, 3136, 1024, 4096): 'gemm_tn8_kernel<1> grid=(1024,1) block=256 lds=65536 chunks=4 rows=896 xcd=1 swapped=0 split=2',
    (0, 9856, 768, 768): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(462,1) block=256 lds=65536',
    (4, 9856, 768, 768): 'gemm_tn_kernel<1, 1, 64> grid=(36,14) block=256 lds=65536 chunks=14 rows=704 xcd=0 swapped=0',
    (0, 9856, 2304, 768): 'gemm_nt_kernel<256, 192, 64, 4, 2, 0> grid=(468,1) block=512 lds=114688',
    (4, 9856, 2304, 768): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=4 rows=2496 xcd=2 swapped=0',
    (0, 9856, 3072, 768): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(468,1) block=512 lds=131072',
    (4, 9856, 3072, 768): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=3 rows=3328 xcd=2 swapped=0',
    (0, 9856, 768, 3072): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(462,1) block=256 lds=65536',
    (4, 9856, 768, 3072): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=3 rows=3328 xcd=1 swapped=0',
    (0, 9856, 768, 2304): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(462,1) block=256 lds=65536',
    (4, 9856, 768, 2304): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=4 rows=2496 xcd=1 swapped=0',
    (0, 12608, 768, 768): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(150,1) block=512 lds=131072',
    (4, 12608, 768, 768): 'gemm_tn_kernel<1, 1, 64> grid=(36,14) block=256 lds=65536 chunks=14 rows=960 xcd=0 swapped=0',
    (0, 12608, 2304, 768): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(450,1) block=512 lds=131072',
    (4, 12608, 2304, 768): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=4 rows=3200 xcd=2 swapped=0',
    (0, 12608, 3072, 768): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(600,1) block=512 lds=131072',
    (4, 12608, 3072, 768): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=3 rows=4224 xcd=2 swapped=0',
    (0, 12608, 768, 3072): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(150,1) block=512 lds=131072',
    (4, 12608, 768, 3072): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=3 rows=4224 xcd=1 swapped=0',
    (0, 12608, 768, 2304): 'gemm_nt_kernel<256, 256, 64, 4, 2, 0> grid=(150,1) block=512 lds=131072',
    (4, 12608, 768, 2304): 'gemm_tn_kernel<1, 1, 64> grid=(432,1) block=256 lds=65536 chunks=4 rows=3200 xcd=1 swapped=0',
    (0, 128, 512, 768): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(4,1) block=256 lds=65536',
    (4, 128, 512, 768): 'gemm_tn_kernel<1, 1, 64> grid=(64,1) block=256 lds=65536 chunks=2 rows=64 xcd=1 swapped=0',
    (0, 128, 256, 768): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(2,1) block=256 lds=65536',
    (4, 128, 256, 768): 'gemm_tn_kernel<1, 1, 64> grid=(32,1) block=256 lds=65536 chunks=2 rows=64 xcd=1 swapped=0',
    (0, 128, 512, 1024): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(4,1) block=256 lds=65536',
    (4, 128, 512, 1024): 'gemm_tn_kernel<1, 1, 64> grid=(64,1) block=256 lds=65536 chunks=2 rows=64 xcd=1 swapped=0',
    (0, 128, 512, 512): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(4,1) block=256 lds=65536',
    (4, 128, 512, 512): 'gemm_tn_kernel<1, 1, 64> grid=(32,1) block=256 lds=65536 chunks=2 rows=64 xcd=1 swapped=0',
    (0, 128, 256, 512): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(2,1) block=256 lds=65536',
    (4, 128, 256, 512): 'gemm_tn_kernel<1, 1, 64> grid=(16,1) block=256 lds=65536 chunks=2 rows=64 xcd=1 swapped=0',
    (0, 128, 768, 512): 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(6,1) block=256 lds=65536',
    (4, 128, 768, 512): 'gemm_tn_kernel<1, 1, 64> grid=(64,1) block=256 lds=65536 chunks=2 rows=64 xcd=2 swapped=0',
}

# (knob, value, (op, M, N, K)) -> plan: the four knobs the entry points read on every call
LIVE_KNOBS = [
    ('MMG_TN_WIDE8', '0', (4, 65536, 192, 384), 'gemm_tn_kernel<1, 1, 64> grid=(480,1) block=256 lds=65536 chunks=79 rows=832 xcd=1 swapped=0'),
    ('MMG_TN8_WIDE', '0', (5, 8192, 256, 256), 'gemm_tn8_kernel<1> grid=(256,1) block=256 lds=65536 chunks=64 rows=128 xcd=1 swapped=0 split=1'),
    ('MMG_TN8_WIDE', '1', (5, 384, 128, 256), 'gemm_tn8_wide_kernel<1> grid=(8,1) block=512 lds=131072 chunks=3 rows=128 xcd=1 swapped=0 split=1'),
    ('MMG_TN8_XCD', '0', (5, 384, 128, 256), 'gemm_tn8_kernel<1> grid=(2,3) block=256 lds=65536 chunks=3 rows=128 xcd=0 swapped=0 split=2'),
    ('MMG_GEMM_192', '0', (0, 21800, 384, 384), 'gemm_nt_kernel<128, 128, 64, 2, 2, 0> grid=(513,1) block=256 lds=65536'),
]


def _plan(op, M, N, K):
    lib = _hip.load()
    return lib.mmg_gemm_plan(op, M, N, K, CUS).decode()


def test_selection_table():
    """Expected strings were recorded from the commit BEFORE the planning layer existed: its four GEMM sources built host-only into a scratch
    library whose launchers' kernel notes were extended with grid, block, LDS and the split fields, its entry points called without a device."""
    wrong = {s: (_plan(*s), want) for s, want in SELECTION.items() if _plan(*s) != want}
    assert not wrong, wrong


@pytest.mark.parametrize("knob,value,shape,want", LIVE_KNOBS, ids=[f"{k}={v}" for k, v, _, _ in LIVE_KNOBS])
def test_live_knobs(monkeypatch, knob, value, shape, want):
    """Recorded like the selection table, with the variable set for the recording run."""
    assert _plan(*shape) == SELECTION[shape] != want
    monkeypatch.setenv(knob, value)
    assert _plan(*shape) == want
    monkeypatch.delenv(knob)
    assert _plan(*shape) == SELECTION[shape]


PLAN_RE = re.compile(r"^(gemm_\w+)<([\d, ]+)> grid=\((\d+),(\d+)\) block=(\d+) lds=(\d+)"
                     r"(?: chunks=(\d+) rows=(\d+) xcd=(\d+) swapped=([01]))?(?: split=(\d+))?$")


def _cdiv(a, b):
    return -(-a // b)


def test_invariants_over_a_shape_sweep():
    """Whatever the shape: a launchable grid and block, LDS within the CU's 160 KiB, the tile grid covers the output, the chunks cover the
    reduction in whole LDS stages.  Shapes an entry point rejects give "" and that entry point's error."""
    lib = _hip.load()
    sizes = (8, 96, 128, 192, 200, 256, 384, 392, 768, 3072)
    valid = 0
    for M in (1, 37, 4095, 4096, 65535, 65536, 4194304 + 17):
        for N in sizes:
            for K in sizes:
                for op in range(7):
                    text = _plan(op, M, N, K)
                    where = (op, M, N, K, text)
                    if not text:
                        assert lib.mmg_last_error().decode().startswith(DOORS[op] + ":"), where
                        continue
                    valid += 1
                    m = PLAN_RE.match(text)
                    assert m, where
                    family, params = m.group(1), [int(x) for x in m.group(2).split(",")]
                    gx, gy, block, lds = (int(m.group(i)) for i in (3, 4, 5, 6))
                    assert 1 <= gx <= 2 ** 31 - 1 and 1 <= gy <= 65535 and block in (256, 512), where
                    assert 0 < lds <= 160 * 1024, where
                    if op < 4:
                        assert family == "gemm_nt_kernel" and m.group(7) is None, where
                        assert gx == _cdiv(M, params[0]) * _cdiv(N, params[1]) and gy == 1, where
                        assert K % (params[2] * (2 if op else 1)) == 0, where          # whole K tiles (8-bit rows: 2 bytes per staged element)
                        continue
                    chunks, rows, swapped = int(m.group(7)), int(m.group(8)), int(m.group(10))
                    n1, n2 = (K, N) if swapped else (N, K)
                    t1, t2, stage = {"gemm_tn_kernel": lambda p: (128 * p[0], 128 * p[1], p[2]), "gemm_tn_wide_kernel": lambda p: (p[0], p[1], 32),
                                     "gemm_tn8_kernel": lambda p: (128, 128, 128), "gemm_tn8_wide_kernel": lambda p: (256, 256, 128)}[family](params)
                    assert chunks >= 1 and chunks * rows >= M and rows % stage == 0, where
                    assert gx * gy >= _cdiv(n1, t1) * _cdiv(n2, t2) * chunks, where
                    assert (m.group(11) is not None) == (op >= 5), where
    assert valid > 2000


@pytest.mark.parametrize("op,M,N,K", [(0, 128, 128, 48), (0, 128, 12, 64), (0, 0, 128, 64), (1, 128, 128, 64), (1, 128, 132, 128), (2, 128, 128, 64),
                                      (3, -1, 128, 128), (4, 128, 4, 128), (4, 128, 128, 100), (4, 0, 128, 128), (5, 128, 24, 128), (6, 128, 128, 8)])
def test_rejected_shapes_give_no_plan_and_the_entry_points_error(op, M, N, K):
    lib = _hip.load()
    assert _plan(op, M, N, K) == ""
    message = lib.mmg_last_error().decode()
    assert message.startswith(DOORS[op] + ":"), message
    assert "launch failed" not in message


def test_unknown_op_gives_no_plan():
    lib = _hip.load()
    assert _plan(7, 128, 128, 128) == "" and lib.mmg_last_error().decode().startswith("mmg_gemm_plan:")
