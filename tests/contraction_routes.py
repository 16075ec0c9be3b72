"""The route ledger of the contraction kernels: plain data, no code.

A route key is what tests/route_ledger.py keeps of one recorded launch: the kernel instantiation as cn_prof_name
spells it, then the facts of the launch description that select a code path (group count, parity classes, strides,
taps, K split, interleave, statistics rows / finalize, double buffering, slice mode), then what only the caller knows
("ws" / "atomics": split-K workspace registered or not, "acc": accumulate, "sink active", "ws full|mid|one|none": the
weight-gradient workspace).

COMPILED     every instantiation of FAMILIES in the built library (tests/test_contraction_routes.py compares it with
             the symbol table). cn_pretime_kernel is recorded under the name <PASS[, reg]>; its key starts with the
             instantiation the launch description states and keeps that name second.
CASES        exact-case id -> part -> the route keys that part emits. Every exact contraction check runs inside the
             recorder and fails with "route changed" when a dispatch rule moves it.
PRODUCTION   configuration id -> phase -> the route keys of one training step (the second), one eval forward and the
             predict forward, as tests/test_contraction_routes_gpu.py records them.
UNREACHABLE  instantiation -> "<file>, <function>: `<condition>` ..." that no argument set the C ABI accepts satisfies.

The GPU run prints every entry in this form (pytest -s: lines starting LEDGER / PRODUCTION).
"""
FAMILIES = ('cn_conv_igemm_vec_kernel',
            'cn_conv_igemm_kernel',
            'cn_wgrad_vec_kernel',
            'cn_wgrad_vec3_kernel',
            'cn_wgrad_kernel',
            'cn_bconv_kernel',
            'cn_bwgrad_kernel',
            'cn_gemm1x1_kernel',
            'cn_pretime_kernel')

COMPILED = [
    'cn_bconv_kernel<1, 10, 2, 4>',
    'cn_bconv_kernel<1, 10, 4, 4>',
    'cn_bconv_kernel<1, 10, 8, 4>',
    'cn_bconv_kernel<1, 4, 2, 4>',
    'cn_bconv_kernel<1, 6, 2, 4>',
    'cn_bconv_kernel<1, 6, 4, 4>',
    'cn_bconv_kernel<2, 10, 2, 2>',
    'cn_bconv_kernel<2, 10, 2, 4>',
    'cn_bconv_kernel<2, 10, 4, 2>',
    'cn_bconv_kernel<2, 10, 4, 4>',
    'cn_bconv_kernel<2, 10, 8, 2>',
    'cn_bconv_kernel<2, 10, 8, 4>',
    'cn_bconv_kernel<2, 4, 2, 2>',
    'cn_bconv_kernel<2, 4, 2, 4>',
    'cn_bconv_kernel<2, 6, 2, 2>',
    'cn_bconv_kernel<2, 6, 2, 4>',
    'cn_bconv_kernel<2, 6, 4, 2>',
    'cn_bconv_kernel<2, 6, 4, 4>',
    'cn_bconv_kernel<4, 10, 2, 4>',
    'cn_bconv_kernel<4, 10, 4, 4>',
    'cn_bconv_kernel<4, 10, 8, 4>',
    'cn_bconv_kernel<4, 4, 2, 4>',
    'cn_bconv_kernel<4, 6, 2, 4>',
    'cn_bconv_kernel<4, 6, 4, 4>',
    'cn_bwgrad_kernel<1, 0, false>',
    'cn_bwgrad_kernel<1, 0, true>',
    'cn_bwgrad_kernel<1, 4, false>',
    'cn_bwgrad_kernel<1, 4, true>',
    'cn_bwgrad_kernel<1, 8, false>',
    'cn_bwgrad_kernel<1, 8, true>',
    'cn_bwgrad_kernel<9, 0, false>',
    'cn_bwgrad_kernel<9, 0, true>',
    'cn_bwgrad_kernel<9, 16, false>',
    'cn_bwgrad_kernel<9, 16, true>',
    'cn_bwgrad_kernel<9, 8, false>',
    'cn_bwgrad_kernel<9, 8, true>',
    'cn_conv_igemm_kernel<1, 1, 12>',
    'cn_conv_igemm_kernel<1, 1, 3>',
    'cn_conv_igemm_kernel<1, 1, 6>',
    'cn_conv_igemm_kernel<1, 2, 12>',
    'cn_conv_igemm_kernel<1, 2, 3>',
    'cn_conv_igemm_kernel<1, 2, 6>',
    'cn_conv_igemm_kernel<2, 2, 12>',
    'cn_conv_igemm_kernel<2, 2, 3>',
    'cn_conv_igemm_kernel<2, 2, 6>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 1, 0>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 2, 0>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 2, 1>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 2, 2>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 2, 3>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 4, 0>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 4, 1>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 4, 2>',
    'cn_conv_igemm_vec_kernel<1, 1, 2, 4, 3>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 1, 0>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 1, 1>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 2, 0>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 2, 1>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 2, 2>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 2, 3>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 4, 0>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 4, 1>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 4, 2>',
    'cn_conv_igemm_vec_kernel<1, 2, 2, 4, 3>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 1, 0>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 1, 2>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 2, 0>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 2, 1>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 2, 2>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 2, 3>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 4, 0>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 4, 1>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 4, 2>',
    'cn_conv_igemm_vec_kernel<2, 2, 2, 4, 3>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 1, 0>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 1, 1>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 2, 0>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 2, 1>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 2, 2>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 2, 3>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 4, 0>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 4, 1>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 4, 2>',
    'cn_conv_igemm_vec_kernel<4, 1, 3, 4, 3>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 1, 0>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 1, 1>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 2, 0>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 2, 1>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 2, 2>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 2, 3>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 4, 0>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 4, 1>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 4, 2>',
    'cn_conv_igemm_vec_kernel<4, 1, 5, 4, 3>',
    'cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>',
    'cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>',
    'cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',
    'cn_gemm1x1_kernel<1, 2, 1, 32, 0, 4>',
    'cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>',
    'cn_gemm1x1_kernel<1, 2, 1, 32, 2, 4>',
    'cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>',
    'cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>',
    'cn_gemm1x1_kernel<2, 2, 1, 32, 2, 3>',
    'cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>',
    'cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>',
    'cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>',
    'cn_pretime_kernel<0, 4, 1, 1, 0, 0>',
    'cn_pretime_kernel<0, 4, 1, 1, 3, 12>',
    'cn_pretime_kernel<0, 4, 2, 1, 0, 0>',
    'cn_pretime_kernel<0, 8, 1, 1, 0, 0>',
    'cn_pretime_kernel<0, 8, 2, 1, 0, 0>',
    'cn_pretime_kernel<1, 4, 1, 1, 0, 0>',
    'cn_pretime_kernel<1, 4, 1, 1, 3, 12>',
    'cn_pretime_kernel<1, 4, 2, 1, 0, 0>',
    'cn_pretime_kernel<1, 8, 1, 1, 0, 0>',
    'cn_pretime_kernel<1, 8, 2, 1, 0, 0>',
    'cn_pretime_kernel<2, 4, 1, 1, 0, 0>',
    'cn_pretime_kernel<2, 4, 1, 1, 3, 12>',
    'cn_pretime_kernel<2, 4, 1, 1, 4, 25>',
    'cn_pretime_kernel<2, 4, 2, 1, 0, 0>',
    'cn_pretime_kernel<2, 8, 1, 1, 0, 0>',
    'cn_pretime_kernel<2, 8, 2, 1, 0, 0>',
    'cn_pretime_kernel<3, 4, 1, 1, 0, 0>',
    'cn_pretime_kernel<3, 4, 1, 1, 3, 12>',
    'cn_pretime_kernel<3, 8, 1, 1, 0, 0>',
    'cn_pretime_kernel<4, 4, 1, 1, 0, 0>',
    'cn_pretime_kernel<4, 4, 1, 1, 3, 12>',
    'cn_pretime_kernel<4, 4, 1, 2, 0, 0>',
    'cn_pretime_kernel<4, 8, 1, 1, 0, 0>',
    'cn_pretime_kernel<4, 8, 1, 2, 0, 0>',
    'cn_pretime_kernel<5, 4, 1, 1, 0, 0>',
    'cn_pretime_kernel<5, 4, 1, 1, 3, 12>',
    'cn_pretime_kernel<5, 8, 1, 1, 0, 0>',
    'cn_wgrad_kernel<1>',
    'cn_wgrad_kernel<9>',
    'cn_wgrad_vec3_kernel<1>',
    'cn_wgrad_vec3_kernel<2>',
    'cn_wgrad_vec_kernel<1, 1>',
    'cn_wgrad_vec_kernel<1, 2>',
]

CASES = {
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x40x12x12x129b-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x40x12x12x129b-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x128x16x20x300-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x128x16x20x300-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x130x9x12x128b-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x130x9x12x128b-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[1x161x8x8x64-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[1x161x8x8x64-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x8x4x4x32b-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x8x4x4x32b-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x7x6x6x33-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x7x6x6x33-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[1x33x5x8x65b-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[1x33x5x8x65b-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x40x13x13x128b-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x40x13x13x128b-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x24x7x6x48-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[2x24x7x6x48-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[3x130x9x11x128b-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[3x130x9x11x128b-none]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x128x25x25x1152b-ws]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x128x25x25x1152b-none]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x1152x25x25x128-ws]': {
        'y': [('cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x1152x25x25x128-none]': {
        'y': [('cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x256x13x13x256b-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x256x13x13x256b-none]': {
        'y': [('cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x576x50x50x128-ws]': {
        'y': [('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x576x50x50x128-none]': {
        'y': [('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x40x63x80x129b-ws]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x40x63x80x129b-none]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x128x72x72x300-ws]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x128x72x72x300-none]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x72x12x12x256b-ws]': {
        'y': [('cn_gemm1x1_kernel<1, 2, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact[8x72x12x12x256b-none]': {
        'y': [('cn_gemm1x1_kernel<1, 2, 1, 32, 0, 4>', 'atomics')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'atomics')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_accumulate[2x40x12x12x129b]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_accumulate[2x128x16x20x300]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_accumulate[1x161x8x8x64]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_accumulate[2x40x13x13x128b]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_accumulate[3x130x9x11x128b]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_accumulate[8x256x13x13x256b]': {
        'y': [('cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_accumulate[8x40x63x80x129b]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[False-case0-1-3]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[False-case1-1-3]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[False-case2-4-8]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[False-case3-2-5]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[False-case4-3-1]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[False-case5-1-3]': {
        'y': [('cn_gemm1x1_kernel<1, 2, 1, 32, 2, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 2, 1, 32, 2, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[False-case6-1-3]': {
        'y': [('cn_gemm1x1_kernel<2, 2, 1, 32, 2, 3>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 2, 3>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[True-case0-1-3]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[True-case1-1-3]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[True-case2-4-8]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[True-case3-2-5]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[True-case4-3-1]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[True-case5-1-3]': {
        'y': [('cn_gemm1x1_kernel<1, 2, 1, 32, 2, 4>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<1, 2, 1, 32, 2, 4>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_padded_batch_strides[True-case6-1-3]': {
        'y': [('cn_gemm1x1_kernel<2, 2, 1, 32, 2, 3>', 'ws', 'acc')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 2, 3>', 'ws', 'acc')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_bias_off_and_on[2x40x12x12x129b]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_bias_off_and_on[2x8x4x4x32b]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_bias_off_and_on[2x40x13x13x128b]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'ws')],
    },
    'test_conv1x1_gemm_exact_gpu.py::test_conv1x1_gemm_exact_bias_off_and_on[8x128x25x25x1152b]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>', 'ws')],
    },
    'test_slice_sums_exact_gpu.py::test_f32_weight_gradient_deferred_exact[case0-flat]': {
        'dw 0 f32': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_weight_gradient_deferred_exact[case1-waves]': {
        'dw 0 f32': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_weight_gradient_deferred_exact[case2-flat]': {
        'dw 0 f32': [
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_weight_gradient_deferred_exact[case3-flat]': {
        'dw 0 f32': [
            ('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_weight_gradient_deferred_exact[case4-flat]': {
        'dw 0 f32': [
            ('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_below_16_slices_under_a_sink_exact[f32-case0-1]': {
        'dw': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_below_16_slices_under_a_sink_exact[f32g-case1-2]': {
        'dw': [
            ('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_below_16_slices_under_a_sink_exact[f32-case2-1]': {
        'dw': [
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_below_16_slices_under_a_sink_exact[f32-case3-1]': {
        'dw': [
            ('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_grouped_weight_gradient_deferred_exact[2]': {
        'dw 0 f32g': [
            ('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_f32_grouped_weight_gradient_deferred_exact[4]': {
        'dw 0 f32g': [
            ('cn_wgrad_vec3_kernel<1>', 'G4', 's1', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case0-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case1-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case2-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'whole', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case3-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<1, 4, true>', 's1', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case4-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case5-one]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'whole', 'sink active', 'ws one')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case6-mid]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'sink active', 'ws mid')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case7-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case8-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case9-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 0, true>', 's2', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_weight_gradient_deferred_exact[case10-full]': {
        'dw 0 bf16': [('cn_bwgrad_kernel<9, 16, false>', 's4', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_bf16_transposed_weight_gradient_deferred_exact': {
        'dw 0 bf16t': [('cn_bwgrad_kernel<9, 8, false>', 's2', 'split', 'sink active', 'ws full')],
    },
    'test_slice_sums_exact_gpu.py::test_mixed_flush_exact': {
        'dw 0 f32': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
        'dw 1 bf16': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'sink active', 'ws full')],
        'dw 2 f32': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
        'dw 3 bf16': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'sink active', 'ws full')],
        'dw 4 bf16': [('cn_bwgrad_kernel<1, 4, true>', 's1', 'split', 'sink active', 'ws full')],
        'dw 5 f32': [
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'sink active', 'ws full'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-100-100-40-3-2-1-1-0]': {
        'y': [('cn_conv_igemm_kernel<1, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-12-12-128-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-12-12-40-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-12-12-8-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-13-13-128-3-2-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-28-28-128-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-3-101-8-3-1-5-5-0]': {
        'y': [('cn_conv_igemm_kernel<1, 1, 6>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 6>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-3-301-128-3-1-2-2-0]': {
        'y': [('cn_conv_igemm_kernel<2, 2, 12>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 12>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-4-256-128-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 2, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-4-512-40-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 4, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-4-512-8-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-5-205-128-3-1-2-2-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-5-205-40-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-5-205-40-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 4, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-5-205-8-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-5-205-8-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-6-101-40-3-1-5-5-0]': {
        'y': [('cn_conv_igemm_kernel<1, 2, 12>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 12>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-6-101-8-3-1-5-5-0]': {
        'y': [('cn_conv_igemm_kernel<1, 1, 12>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 12>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-6-510-40-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 4, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-6-510-8-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-128-128-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 2, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-128-40-3-1-2-2-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 2, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-128-40-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 2, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-128-8-3-1-2-2-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-128-8-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-130-40-3-1-2-2-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 2, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-255-40-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 4, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-255-8-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 4, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[1-8-8-258-128-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 2, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[32-8-5-205-128-3-1-2-2-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[32-8-8-129-128-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[32-8-8-129-128-3-1-5-5-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 2, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 0>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[32-8-8-130-128-3-1-2-2-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 2, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_ledger_cases[8-72-8-258-128-3-1-1-1-0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 2, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 2, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case1]': {
        'y': [('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case2]': {
        'y': [('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case3]': {
        'y': [('cn_conv_igemm_kernel<1, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case4]': {
        'y': [('cn_conv_igemm_kernel<1, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws')],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'whole', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case5]': {
        'y': [('cn_conv_igemm_kernel<2, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws')],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case6]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case7]': {
        'y': [('cn_conv_igemm_kernel<2, 2, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws')],
        'dw': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case8]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case9]': {
        'y': [('cn_conv_igemm_kernel<2, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws')],
        'dx': [('cn_conv_igemm_kernel<1, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws')],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case10]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case11]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws')],
        'dw': [('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case12]': {
        'y': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>', 'ws')],
        'dw': [('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case13]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case14]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case15]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case16]': {
        'y': [('cn_conv_igemm_kernel<2, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws')],
        'dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case17]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case18]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 1>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact[case19]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il0', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_atomic_split[case0]': {
        'y': [
            ('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'atomics'),
        ],
        'dx': [
            ('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'atomics'),
        ],
        '+= y': [
            ('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'atomics'),
        ],
        '+= dx': [
            ('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_atomic_split[case1]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'atomics'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'atomics'),
        ],
        '+= y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'atomics'),
        ],
        '+= dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_atomic_split[case2]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        '+= y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        '+= dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_atomic_split[case3]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        '+= y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        '+= dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_accumulate_padded_strides[case0-4-8]': {
        '+= y': [
            ('cn_conv_igemm_kernel<1, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'xpad4 ypad8'),
        ],
        '+= dx': [
            ('cn_conv_igemm_kernel<1, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'xpad4 ypad8'),
        ],
        '+= dw': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'xpad4 ypad8', 'ws full'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_accumulate_padded_strides[case1-3-5]': {
        '+= y': [
            ('cn_conv_igemm_kernel<2, 2, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws', 'xpad3 ypad5'),
        ],
        '+= dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws', 'xpad3 ypad5'),
        ],
        '+= dw': [
            ('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'ws', 'xpad3 ypad5', 'ws full'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_accumulate_padded_strides[case2-8-1]': {
        '+= y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'xpad8 ypad1'),
        ],
        '+= dx': [
            ('cn_conv_igemm_kernel<1, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'xpad8 ypad1'),
        ],
        '+= dw': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'xpad8 ypad1', 'ws full'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_accumulate_padded_strides[case3-3-0]': {
        '+= y': [
            ('cn_conv_igemm_kernel<1, 2, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'xpad3 ypad0'),
        ],
        '+= dx': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'xpad3 ypad0'),
        ],
        '+= dw': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'xpad3 ypad0', 'ws full'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_1x1_gemm[case0]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws')],
        '+= y': [('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_1x1_gemm[case1]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws')],
        '+= y': [('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_1x1_gemm[case2]': {
        'y': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws')],
        'dx': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws')],
        '+= y': [('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_production_100[case0]': {
        'y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 1>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case0]': {
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case1]': {
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case2]': {
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case3]': {
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case4]': {
        'dw': [('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case5]': {
        'dw': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case6]': {
        'dw': [('cn_wgrad_vec_kernel<1, 2>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case7]': {
        'dw': [('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[full-case8]': {
        'dw': [('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'whole', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case0]': {
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case1]': {
        'dw': [('cn_wgrad_kernel<9>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case2]': {
        'dw': [('cn_wgrad_kernel<9>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case3]': {
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case4]': {
        'dw': [('cn_wgrad_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case5]': {
        'dw': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case6]': {
        'dw': [('cn_wgrad_vec_kernel<1, 2>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case7]': {
        'dw': [('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_routes[none-case8]': {
        'dw': [('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'whole', 'atomics', 'ws none')],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_weight_gradient_padded_batch_stride': {
        'ws full: dw': [
            ('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'xpad1 ypad3', 'ws full'),
        ],
        'ws none: dw': [
            ('cn_wgrad_kernel<9>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'xpad1 ypad3', 'ws none'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_f32_exact_largest_weight_gradient': {
        'dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case0]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case1]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 2>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf2', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case2]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws', 'acc'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case3]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_kernel<1, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices')],
        'transposed dw ws none': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case4]': {
        'transposed y': [
            ('cn_conv_igemm_kernel<1, 2, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws', 'acc'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf2', 'whole', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case5]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls16', 'is1', 'os4', 'taps1', 'whole', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls1', 'is4', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_kernel<9>', 'G1', 's4', 'nbuf1', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's4', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case6]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case7]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case8]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_kernel<2, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices')],
        'transposed dw ws none': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case9]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case10]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 1>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case11]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il0', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case12]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_kernel<1, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case13]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_kernel<2, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf1', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case14]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_kernel<1, 1, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'slices')],
        'transposed dw ws none': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case15]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il0', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'slices')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf2', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_exact[case16]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il0', 'ws'),
        ],
        'transposed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 2, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'transposed dw ws full': [('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf2', 'split', 'slices')],
        'transposed dw ws none': [('cn_wgrad_kernel<9>', 'G1', 's2', 'nbuf2', 'split', 'atomics')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[1-8-4-511-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 2, 0>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[1-8-4-256-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 2, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[1-8-5-409-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 2, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[1-8-4-1022-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 4, 0>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[1-8-4-512-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 4, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[1-8-4-510-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 4, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[1-8-3-683-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 4, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[1-72-4-1022-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 4, 0>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[2-72-4-512-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 4, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[2-72-4-510-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 4, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[4-8-3-683-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 4, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[64-8-8-256-72]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 2, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[32-8-4-1022-72]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 4, 0>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[64-8-4-512-72]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 4, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[64-8-4-510-72]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 4, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[8-8-3-683-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 4, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_f32_forward_wide_exact[16-8-5-205-128]': {
        'transposed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
        ],
    },
    'test_conv_exact_gpu.py::test_convt_taps_route_exact[2-16-7-7]': {
        'engine forward': [('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>',)],
        'engine backward': [
            ('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>',),
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_convt_taps_route_exact[1-9-25-25]': {
        'engine forward': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',)],
        'engine backward': [
            ('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',),
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_convt_taps_route_exact[2-3-5-6]': {
        'engine forward': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',)],
        'engine backward': [
            ('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',),
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_time_conv_exact[3]': {
        'engine forward': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',)],
        'engine backward': [
            ('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',),
            ('cn_wgrad_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_time_conv_exact[5]': {
        'engine forward': [('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',)],
        'engine backward': [
            ('cn_gemm1x1_kernel<1, 1, 1, 32, 2, 4>',),
            ('cn_wgrad_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics'),
        ],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[1-2-16-13-13-24-dils0-False-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G1', 'cls1', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-2-24-14-14-32-dils1-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[3-1-9-11-7-33-dils2-False-ws]': {
        'grouped y': [
            ('cn_conv_igemm_kernel<1, 2, 3>', 'G>1', 'cls3', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_kernel<1, 2, 3>', 'G>1', 'cls3', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_kernel<1, 1, 3>', 'G>1', 'cls3', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_kernel<1, 1, 3>', 'G>1', 'cls3', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G3', 's1', 'nbuf2', 'whole', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[4-2-32-25-25-64-dils3-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls4', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls4', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G>1', 'cls4', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G>1', 'cls4', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G4', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-8-128-25-25-128-dils4-True-none]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[3-2-64-7-7-128-dils5-False-none]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G>1', 'cls3', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G>1', 'cls3', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls3', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls3', 'is1', 'os1', 'taps9', 'split', 'il0', 'atomics'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G3', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-8-32-100-100-32-dils6-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-8-64-50-50-64-dils7-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-8-128-50-50-128-dils8-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-8-128-25-25-128-dils9-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-4-64-55-55-64-dils10-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-4-128-28-28-128-dils11-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-4-128-55-55-128-dils12-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-1-8-13-13-40-dils13-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-16-8-28-28-128-dils14-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-1-8-13-13-128-dils15-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-1-8-14-14-128-dils16-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-4-8-100-100-128-dils17-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_grouped_f32_exact[2-16-8-50-50-128-dils18-True-ws]': {
        'grouped y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed y': [
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws', 'acc'),
        ],
        'grouped dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped summed dx': [
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
        ],
        'grouped dw': [('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case0]': {
        'y': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case1]': {
        'y': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case2]': {
        'y': [('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'whole', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case3]': {
        'y': [('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case4]': {
        'y': [('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'whole', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case5]': {
        'y': [('cn_bconv_kernel<2, 6, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case6]': {
        'y': [('cn_bconv_kernel<2, 4, 2, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 4, 2, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case7]': {
        'y': [('cn_bconv_kernel<2, 10, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case8]': {
        'y': [('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case9]': {
        'y': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'whole', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case10]': {
        'y': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case11]': {
        'y': [('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case12]': {
        'y': [('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case13]': {
        'y': [('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case14]': {
        'y': [('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact[case15]': {
        'y': [('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_accumulate[case0]': {
        'y': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'y f32 out': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'dx': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_accumulate[case1]': {
        'y': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'y f32 out': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'dx': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_accumulate[case2]': {
        'y': [
            ('cn_bconv_kernel<2, 6, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'dx': [
            ('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_accumulate[case3]': {
        'y': [
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'dx': [
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_accumulate[case4]': {
        'y': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'dx': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[full-case0]': {
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[full-case1]': {
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[full-case2]': {
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[full-case3]': {
        'dw': [('cn_bwgrad_kernel<1, 4, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[mid-case0]': {
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws mid')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[mid-case1]': {
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws mid')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[mid-case2]': {
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's2', 'whole', 'ws mid')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[mid-case3]': {
        'dw': [('cn_bwgrad_kernel<1, 4, true>', 's1', 'split', 'ws mid')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[one-case0]': {
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'whole', 'ws one')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[one-case1]': {
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'whole', 'ws one')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[one-case2]': {
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's2', 'whole', 'ws one')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_weight_gradient_workspaces[one-case3]': {
        'dw': [('cn_bwgrad_kernel<1, 4, true>', 's1', 'whole', 'ws one')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-8-5-6-8-3-1-5-5-0]': {
        'y': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-40-5-6-8-1-1-0-1-1]': {
        'y': [('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[1-8-20-25-8-1-1-0-1-0]': {
        'y': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-40-10-10-8-1-2-0-1-1]': {
        'y': [('cn_bconv_kernel<1, 10, 4, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 10, 4, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls4', 'taps1', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-72-5-6-8-1-1-0-1-0]': {
        'y': [('cn_bconv_kernel<1, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-8-5-6-128-1-1-0-1-1]': {
        'y': [('cn_bconv_kernel<2, 4, 2, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 4, 2, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-8-5-6-40-1-1-0-1-0]': {
        'y': [('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 4, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[1-8-5-6-128-3-1-5-5-1]': {
        'y': [('cn_bconv_kernel<2, 6, 2, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 2, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's1', 'whole', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[1-8-5-6-40-3-1-5-5-0]': {
        'y': [('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's1', 'whole', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-40-5-6-128-1-1-0-1-0]': {
        'y': [('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-40-5-6-40-1-1-0-1-1]': {
        'y': [('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[1-8-10-50-128-1-2-0-1-0]': {
        'y': [('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 8, 4>', 'G1', 'cls4', 'taps1', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 0, true>', 's2', 'whole', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[1-8-10-50-40-1-2-0-1-1]': {
        'y': [('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls4', 'taps1', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 0, true>', 's2', 'whole', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[1-40-10-10-128-1-2-0-1-1]': {
        'y': [('cn_bconv_kernel<2, 10, 4, 2>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 4, 2>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls4', 'taps1', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[1-40-10-10-40-1-2-0-1-0]': {
        'y': [('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls4', 'taps1', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-72-5-6-128-1-1-0-1-1]': {
        'y': [('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-72-5-6-40-1-1-0-1-0]': {
        'y': [('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-8-5-6-256-1-1-0-1-0]': {
        'y': [('cn_bconv_kernel<4, 4, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 4, 2, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-8-5-6-256-3-1-5-5-0]': {
        'y': [('cn_bconv_kernel<4, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-40-5-6-256-1-1-0-1-1]': {
        'y': [('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-40-5-6-256-3-1-1-1-0]': {
        'y': [('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-8-9-49-256-1-2-0-1-0]': {
        'y': [('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 8, 4>', 'G1', 'cls4', 'taps1', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 0, true>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-40-10-10-256-1-2-0-1-0]': {
        'y': [('cn_bconv_kernel<4, 10, 4, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 10, 4, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls4', 'taps1', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[57-40-5-25-512-3-1-2-2-0]': {
        'y': [('cn_bconv_kernel<4, 10, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 10, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-72-5-6-256-1-1-0-1-0]': {
        'y': [('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-16-1-255-24-1-2-0-1-0]': {
        'y': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps1', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls2', 'taps1', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 8, true>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-16-22-22-24-1-3-0-1-0]': {
        'y': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is3', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps1', 'is3', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls9', 'taps1', 'is1', 'os3', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 8, false>', 's3', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-16-29-29-24-1-4-0-1-0]': {
        'y': [('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps1', 'is4', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps1', 'is4', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<1, 0, false>', 's4', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-16-10-25-24-3-1-4-4-0]': {
        'y': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-16-10-25-24-3-1-5-5-0]': {
        'y': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 0, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-16-15-15-24-3-2-4-4-0]': {
        'y': [('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls4', 'taps9', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 0, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[2-32-26-26-64-3-2-1-1-0]': {
        'y': [('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 10, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-40-25-25-128-3-2-1-1-0]': {
        'y': [('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, false>', 's2', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[57-40-17-97-128-3-4-1-1-0]': {
        'y': [('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is4', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is4', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<2, 10, 8, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 16, false>', 's4', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_conv2d_bf16_exact_ledger_cases[113-9-5-25-256-3-1-1-1-0]': {
        'y': [('cn_bconv_kernel<4, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<4, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'dx': [('cn_bconv_kernel<1, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'dw': [('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'ws full')],
    },
    'test_conv_exact_gpu.py::test_bf16_outputs_round_ties_to_even': {
        'y': [('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0')],
        'y f32 out': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
    },
    'test_conv_exact_gpu.py::test_grouped_bf16_exact[1-2-16-13-13-24-dils0-False]': {
        'grouped y': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y +=': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'grouped y no bias': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y bnstats': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1', 'stats rows and finalize requested'),
        ],
        'grouped dx': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped dx +=': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_grouped_bf16_exact[2-2-32-14-14-32-dils1-True]': {
        'grouped y': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y +=': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'grouped y no bias': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y bnstats': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1', 'stats rows and finalize requested'),
        ],
        'grouped dx': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped dx +=': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_grouped_bf16_exact[3-1-24-11-9-40-dils2-False]': {
        'grouped y': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls3', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y +=': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls3', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'grouped y no bias': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls3', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y bnstats': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls3', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1', 'stats rows and finalize requested'),
        ],
        'grouped dx': [
            ('cn_bconv_kernel<1, 10, 4, 4>', 'G>1', 'cls3', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped dx +=': [
            ('cn_bconv_kernel<1, 10, 4, 4>', 'G>1', 'cls3', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_grouped_bf16_exact[4-2-64-25-25-64-dils3-True]': {
        'grouped y': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G>1', 'cls4', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y +=': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G>1', 'cls4', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'grouped y no bias': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G>1', 'cls4', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y bnstats': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G>1', 'cls4', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1', 'stats rows and finalize requested'),
        ],
        'grouped dx': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G>1', 'cls4', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped dx +=': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G>1', 'cls4', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_grouped_bf16_exact[2-2-64-50-50-64-dils4-True]': {
        'grouped y': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y +=': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'grouped y no bias': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y bnstats': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1', 'stats rows and finalize requested'),
        ],
        'grouped dx': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped dx +=': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_grouped_bf16_exact[2-2-40-25-25-128-dils5-True]': {
        'grouped y': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y +=': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'grouped y no bias': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y bnstats': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1', 'stats rows and finalize requested'),
        ],
        'grouped dx': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped dx +=': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_grouped_bf16_exact[2-8-40-50-50-128-dils6-True]': {
        'grouped y': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y +=': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'grouped y no bias': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped y bnstats': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1', 'stats rows and finalize requested'),
        ],
        'grouped dx': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'grouped dx +=': [
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
    },
    'test_conv_exact_gpu.py::test_bnstats_bf16_strided_1x1_refused_exact[1-2-16-26-26-128-3-2-True]': {
        'y bnstats': [
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st1', 'fin1', 'finalize workspace given'),
        ],
    },
    'test_conv_exact_gpu.py::test_bnstats_bf16_strided_1x1_refused_exact[1-2-16-26-26-64-3-2-True]': {
        'y bnstats': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st1', 'fin1', 'finalize workspace given'),
        ],
    },
    'test_conv_exact_gpu.py::test_bnstats_bf16_strided_1x1_refused_exact[1-2-72-13-13-128-1-1-True]': {
        'y bnstats': [
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st1', 'fin1', 'finalize workspace given'),
        ],
    },
    'test_conv_exact_gpu.py::test_bnstats_bf16_strided_1x1_refused_exact[2-113-40-5-6-128-3-1-False]': {
        'y bnstats': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin0', 'finalize workspace withheld'),
        ],
    },
    'test_conv_exact_gpu.py::test_fused_bf16_exact[2-16-13-13-32-3-1-1-1-True]': {
        'fused y': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'res'),
        ],
        'fused y in place': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'res'),
        ],
    },
    'test_conv_exact_gpu.py::test_fused_bf16_exact[1-24-7-5-8-3-2-1-1-False]': {
        'fused y': [
            ('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0', 'no res'),
        ],
    },
    'test_conv_exact_gpu.py::test_fused_bf16_exact[2-64-25-25-128-3-1-2-2-True]': {
        'fused y': [
            ('cn_bconv_kernel<2, 10, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'res'),
        ],
        'fused y in place': [
            ('cn_bconv_kernel<2, 10, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0', 'res'),
        ],
    },
    'test_conv_exact_gpu.py::test_fused_bf16_exact[2-40-10-10-64-1-1-0-1-True]': {
        'fused y': [
            ('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0', 'res'),
        ],
        'fused y in place': [
            ('cn_bconv_kernel<2, 6, 4, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0', 'res'),
        ],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[2-16-13-13-16-2-False]': {
        'transposed y': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 8, false>', 's2', 'split')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 8, false>', 's2', 'whole')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[2-32-25-25-32-2-True]': {
        'transposed y': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0', 'acc'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 0, true>', 's2', 'split')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 0, true>', 's2', 'whole')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[1-128-50-50-128-2-False]': {
        'transposed y': [
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 0, true>', 's2', 'split')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 0, true>', 's2', 'whole')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[2-32-7-7-24-4-False]': {
        'transposed y': [
            ('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is4', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 16, false>', 's4', 'split')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 16, false>', 's4', 'whole')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[1-24-5-6-31-2-True]': {
        'transposed y': [
            ('cn_bconv_kernel<1, 4, 2, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0', 'acc'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<1, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0', 'acc'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 16, false>', 's2', 'whole')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 16, false>', 's2', 'whole')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[1-128-25-25-128-4-False]': {
        'transposed y': [
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is4', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 16, false>', 's4', 'split')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 16, false>', 's4', 'whole')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[4-128-25-25-128-4-False]': {
        'transposed y': [
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is4', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 16, false>', 's4', 'split')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 16, false>', 's4', 'whole')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[32-128-13-13-128-2-False]': {
        'transposed y': [
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 8, false>', 's2', 'split')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 8, false>', 's2', 'whole')],
    },
    'test_conv_exact_gpu.py::test_conv_transpose2d_bf16_exact[2-64-50-50-64-2-False]': {
        'transposed y': [
            ('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
        ],
        'transposed dx': [
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
        ],
        'transposed dw ws full': [('cn_bwgrad_kernel<9, 0, true>', 's2', 'split')],
        'transposed dw ws one': [('cn_bwgrad_kernel<9, 0, true>', 's2', 'whole')],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c5t6-o8-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c5t6-o24-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c5t6-o32-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c8t5-o8-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c8t5-o24-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c8t5-o32-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c6t8-o8-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 2, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c6t8-o24-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 2, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c6t8-o32-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 2, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c4t12-o8-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 4, 1, 2, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c4t12-o24-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 4, 1, 2, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c4t12-o32-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 4, 1, 2, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c4t25-o8-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 4, 25>', 'cn_pretime_kernel<2, reg>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c4t25-o24-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 4, 25>', 'cn_pretime_kernel<2, reg>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c4t25-o32-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 4, 25>', 'cn_pretime_kernel<2, reg>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c3t12-o8-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<0, reg>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<1, reg>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<3, reg>', 'training'),
            ('cn_pretime_kernel<4, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<4, reg>', 'training'),
            ('cn_pretime_kernel<5, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<5, reg>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c3t12-o24-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<0, reg>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<1, reg>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<3, reg>', 'training'),
            ('cn_pretime_kernel<4, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<4, reg>', 'training'),
            ('cn_pretime_kernel<5, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<5, reg>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_dispatch[c3t12-o32-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<0, reg>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<1, reg>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<3, reg>', 'training'),
            ('cn_pretime_kernel<4, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<4, reg>', 'training'),
            ('cn_pretime_kernel<5, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<5, reg>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_wide_outputs[c3t12-o40-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<2>', 'eval'),
            ('cn_pretime_kernel<2, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_wide_outputs[c5t6-o56-bf16]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 2, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 2, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 2, 1, 0, 0>', 'cn_pretime_kernel<2>', 'eval'),
            ('cn_pretime_kernel<2, 8, 2, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_wide_outputs[c4t12-o64-f32]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<2>', 'eval'),
            ('cn_pretime_kernel<2, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_eval_backward[c3t12-o32-f32]': {
        'forward': [('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>', 'eval')],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<3, reg>', 'eval'),
            ('cn_pretime_kernel<4, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<4, reg>', 'eval'),
            ('cn_pretime_kernel<5, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<5, reg>', 'eval'),
        ],
    },
    'test_pretime_exact_gpu.py::test_eval_backward[c6t8-o24-bf16]': {
        'forward': [('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'eval')],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'eval'),
            ('cn_pretime_kernel<4, 8, 1, 2, 0, 0>', 'cn_pretime_kernel<4>', 'eval'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'eval'),
        ],
    },
    'test_pretime_exact_gpu.py::test_more_tiles_than_blocks[reg-c3t12]': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<0, reg>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<1, reg>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<3, reg>', 'training'),
            ('cn_pretime_kernel<4, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<4, reg>', 'training'),
            ('cn_pretime_kernel<5, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<5, reg>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_more_tiles_than_blocks[inf-c4t25]': {
        'forward': [('cn_pretime_kernel<2, 4, 1, 1, 4, 25>', 'cn_pretime_kernel<2, reg>', 'eval')],
    },
    'test_pretime_exact_gpu.py::test_more_tiles_than_blocks[gen-c5t6]': {
        'forward': [
            ('cn_pretime_kernel<0, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 8, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
    'test_pretime_exact_gpu.py::test_small_cube_one_entry_tile': {
        'forward': [
            ('cn_pretime_kernel<0, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<0>', 'training'),
            ('cn_pretime_kernel<1, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<1>', 'training'),
            ('cn_pretime_kernel<2, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<2>', 'training'),
        ],
        'backward': [
            ('cn_pretime_kernel<3, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<3>', 'training'),
            ('cn_pretime_kernel<4, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<4>', 'training'),
            ('cn_pretime_kernel<5, 4, 1, 1, 0, 0>', 'cn_pretime_kernel<5>', 'training'),
        ],
    },
}

PRODUCTION = {
    'train fp32 hidden 32 batch 8': {
        'step': [
            ('cn_conv_igemm_kernel<1, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_kernel<2, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'ws'),
            ('cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>', 'ws'),
            ('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws'),
            ('cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws'),
            ('cn_pretime_kernel<0, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<0, reg>'),
            ('cn_pretime_kernel<1, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<1, reg>'),
            ('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>'),
            ('cn_pretime_kernel<3, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<3, reg>'),
            ('cn_pretime_kernel<4, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<4, reg>'),
            ('cn_pretime_kernel<5, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<5, reg>'),
            ('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'atomics', 'sink active'),
            ('cn_wgrad_vec3_kernel<1>', 'G2', 's1', 'nbuf2', 'split', 'slices', 'sink active'),
            ('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'atomics', 'sink active'),
            ('cn_wgrad_vec3_kernel<2>', 'G1', 's2', 'nbuf1', 'split', 'slices', 'sink active'),
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'sink active'),
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'sink active'),
        ],
        'eval': [
            ('cn_conv_igemm_kernel<1, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_gemm1x1_kernel<1, 1, 1, 32, 1, 4>', 'ws'),
            ('cn_gemm1x1_kernel<1, 2, 1, 32, 1, 4>', 'ws'),
            ('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws'),
            ('cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws'),
            ('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>'),
        ],
    },
    'train bf16-mixed hidden 32 batch 32': {
        'step': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is4', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'sink active'),
            ('cn_bwgrad_kernel<1, 4, true>', 's1', 'split', 'sink active'),
            ('cn_bwgrad_kernel<9, 0, true>', 's2', 'split', 'sink active'),
            ('cn_bwgrad_kernel<9, 16, false>', 's4', 'split', 'sink active'),
            ('cn_bwgrad_kernel<9, 8, false>', 's2', 'split', 'sink active'),
            ('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'sink active'),
            ('cn_pretime_kernel<0, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<0, reg>'),
            ('cn_pretime_kernel<1, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<1, reg>'),
            ('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>'),
            ('cn_pretime_kernel<3, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<3, reg>'),
            ('cn_pretime_kernel<4, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<4, reg>'),
            ('cn_pretime_kernel<5, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<5, reg>'),
        ],
        'eval': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_pretime_kernel<2, 4, 1, 1, 3, 12>', 'cn_pretime_kernel<2, reg>'),
        ],
    },
    'train bf16-mixed hidden 64 batch 4 dropout 0.1': {
        'step': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is4', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 4, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G>1', 'cls2', 'taps9', 'is1', 'os1', 'il0', 'st1', 'fin1'),
            ('cn_bwgrad_kernel<1, 4, false>', 's1', 'split', 'sink active'),
            ('cn_bwgrad_kernel<1, 4, true>', 's1', 'split', 'sink active'),
            ('cn_bwgrad_kernel<9, 0, true>', 's2', 'split', 'sink active'),
            ('cn_bwgrad_kernel<9, 16, false>', 's4', 'split', 'sink active'),
            ('cn_bwgrad_kernel<9, 8, false>', 's2', 'split', 'sink active'),
            ('cn_bwgrad_kernel<9, 8, true>', 's1', 'split', 'sink active'),
            ('cn_gemm1x1_kernel<1, 2, 1, 32, 0, 4>', 'ws'),
            ('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws'),
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'atomics', 'sink active'),
            ('cn_wgrad_vec_kernel<1, 1>', 'G1', 's1', 'nbuf2', 'split', 'slices', 'sink active'),
        ],
        'eval': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_pretime_kernel<2, 4, 2, 1, 0, 0>', 'cn_pretime_kernel<2>'),
        ],
    },
    'predict fp32 4 windows': {
        'forward': [
            ('cn_conv_igemm_kernel<1, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'split', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 1>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_gemm1x1_kernel<1, 1, 1, 32, 0, 4>', 'ws'),
            ('cn_gemm1x1_kernel<1, 2, 1, 32, 0, 4>', 'ws'),
            ('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws'),
            ('cn_gemm1x1_kernel<2, 2, 1, 32, 1, 3>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws'),
            ('cn_pretime_kernel<2, 4, 1, 1, 4, 25>', 'cn_pretime_kernel<2, reg>'),
        ],
    },
    'predict bf16-mixed 4 windows': {
        'forward': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 4, 2>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_pretime_kernel<2, 4, 1, 1, 4, 25>', 'cn_pretime_kernel<2, reg>'),
        ],
    },
    'predict fp32 36 windows': {
        'forward': [
            ('cn_conv_igemm_kernel<1, 2, 6>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 1, 2, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<1, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 1>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<2, 2, 2, 1, 3>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 1>', 'G1', 'cls1', 'is2', 'os1', 'taps9', 'split', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 3, 1, 2>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 2>', 'G>1', 'cls2', 'is1', 'os1', 'taps9', 'whole', 'il0', 'ws'),
            ('cn_conv_igemm_vec_kernel<4, 1, 5, 1, 3>', 'G1', 'cls4', 'is1', 'os2', 'taps4', 'whole', 'il1', 'ws'),
            ('cn_gemm1x1_kernel<2, 2, 1, 32, 0, 3>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 4, 32, 0, 2>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 4, 32, 1, 2>', 'ws'),
            ('cn_gemm1x1_kernel<4, 1, 5, 32, 0, 2>', 'ws'),
            ('cn_pretime_kernel<2, 4, 1, 1, 4, 25>', 'cn_pretime_kernel<2, reg>'),
        ],
    },
    'predict bf16-mixed 36 windows': {
        'forward': [
            ('cn_bconv_kernel<1, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 2>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 10, 8, 2>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<2, 6, 2, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 2, 4>', 'G1', 'cls1', 'taps9', 'is2', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls1', 'taps1', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 10, 8, 4>', 'G1', 'cls16', 'taps1', 'is1', 'os4', 'il1', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls1', 'taps9', 'is1', 'os1', 'il0', 'st0', 'fin0'),
            ('cn_bconv_kernel<4, 6, 4, 4>', 'G1', 'cls4', 'taps4', 'is1', 'os2', 'il1', 'st0', 'fin0'),
            ('cn_pretime_kernel<2, 4, 1, 1, 4, 25>', 'cn_pretime_kernel<2, reg>'),
        ],
    },
}

UNREACHABLE = {}
