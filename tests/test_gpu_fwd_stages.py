"""-m gpu: stage gate of the forward pass -- every stored activation of the default schedule against fp64, per pixel class.

The model runs forward (no autograd edge: the training plan of the shape, which stores every stage) on oracle.closed_form_image with
oracle.closed_form_params; tests/gpu_util.hip_forward_trace reads the stored tensors back and tests/fwd_stage_ref.py judges each one
against the float64 evaluation of ITS stage on the run's own upstream tensors, whole tensor, per pixel class and per plane mean:
  bf16   every entry <= 3 x its budget (the same stage in float32 with the kernels' bf16 rounding points, on the same inputs);
  fp32   every entry <= 2e-5 of own norm, or <= 3 x the float32 oracle's own error;
  sr     bit-equal to clamp(srpre) cropped, in both.
Run with -s for each cell's table (error, budget, ratio per (stage, class)).  The bf16 default tails keep the last GELU in LDS (x4) or
registers (x2 / x3): the stored form runs first, its sr must be bit-equal to the default form's and every tensor both forms store
likewise; t2act / t2der (t1act / t1der) are taken from it.  The clamp is live in every cell and asserted to be.

CELLS.  x4, one block: 1x32x32 (one level-2 window); 2x40x56 (reflect-padded to 64x64); 3x64x96 (odd B, W % 64 != 0: branch_prep_tiled<L, 32>);
1x96x128 (the first interior level-2 window); 1x96x96 (3 x 3 = 9 level-2 windows, an odd count); 2x72x24 (TALL: padded to 96x32, a single
32-pixel strip, 3 x 1 level-2 windows).  x4, two blocks, 2x40x56: the non-last block, the statistics out of the conv's epilogue, the X0
fold in the last block only.  x2 / x3, one block, 2x40x56 and 2x72x24: the streaming tails.  bf16 only: fused_c16_fwd = fused_attn_fwd = 1
(q | k | v of branches 1 and 2 stored and gated, everything else bit-equal to the default run); the plain forward kernels
(fused_attn_fwd = fused_c16_fwd = fused_prep_fwd = conv_rows = fused_tail = 0) at 2x40x56 and 2x72x24; fused_attn_fwd2 = 1 and 2 at 3x64x96
(even window count) and 2 at 1x96x96 (odd: falls back to one window per workgroup).  Not covered: maps of >= 0.5 M pixels, where the rows
conv takes segments of 32 / 64 rows (tests/test_gpu_baseline_configs.py test_config4 has length 32 on whole tensors).

The first device run found no kernel fault and forced no rounding point or accumulation order into the emulation: the kernels round where
the emulation rounds (every bf16 ratio of a stored tensor lies in 0.996 .. 1.007 over all cells and classes), and the statistics kernels
stay within 0.76x .. 1.2x of their float32 restatement.

MEASURED on MI355X, worst over the cells per (stage, class): bf16 = error / budget with (error, budget) and the cell; fp32 = error with
(the float32 oracle's own error) and the cell.  Cells are named <scale> nb<blocks> <B>x<H>x<W> [qkv | plain | fwd2=<variant>].
  stage      class        | bf16: worst error / budget (error, budget), cell             | fp32: worst error (float32 oracle's), cell
  X0         all          |  1.000 (1.6e-03, 1.6e-03) x4 nb1 1x32x32                     | 1.2e-07 (2.4e-07) x4 nb1 2x72x24
  X0         border       |  1.000 (1.7e-03, 1.7e-03) x4 nb1 1x32x32                     | 1.2e-07 (2.4e-07) x4 nb1 2x72x24
  X0         interior     |  1.000 (1.6e-03, 1.6e-03) x4 nb1 1x32x32                     | 1.2e-07 (1.2e-07) x4 nb1 1x32x32
  X0         image        |  1.000 (1.6e-03, 1.6e-03) x4 nb1 1x32x32                     | 1.2e-07 (1.2e-07) x4 nb1 1x32x32
  X0         chan_mean    |  1.004 (1.8e-05, 1.8e-05) x4 nb1 1x96x96                     | 3.8e-09 (8.7e-09) x4 nb1 1x32x32
  b0.mean    all          |  1.001 (3.4e-08, 3.4e-08) x4 nb1 2x72x24                     | 5.3e-08 (5.5e-08) x4 nb1 1x96x128
  b0.rstd    all          |  1.079 (4.5e-08, 4.1e-08) x4 nb1 1x96x96                     | 6.1e-08 (4.3e-08) x4 nb1 2x72x24
  b0.d1      all          |  1.000 (1.7e-03, 1.7e-03) x4 nb1 1x32x32                     | 1.1e-07 (9.5e-08) x4 nb1 1x96x128
  b0.d1      img_border   |  1.000 (1.7e-03, 1.7e-03) x4 nb1 1x32x32                     | 1.3e-07 (1.1e-07) x4 nb1 1x96x128
  b0.d1      cover1       |  1.000 (1.7e-03, 1.7e-03) x4 nb1 1x32x32                     | 1.1e-07 (9.4e-08) x4 nb1 1x96x128
  b0.d1      cover2       |  1.000 (1.7e-03, 1.7e-03) x4 nb1 1x32x32                     | 1.1e-07 (9.4e-08) x4 nb1 1x96x128
  b0.d1      cover4       |  1.000 (1.6e-03, 1.6e-03) x4 nb1 1x32x32                     | 1.1e-07 (9.4e-08) x4 nb1 1x96x128
  b0.d1      image        |  1.000 (1.7e-03, 1.7e-03) x4 nb1 1x32x32                     | 1.1e-07 (9.5e-08) x4 nb1 1x96x128
  b0.d1      chan_mean    |  1.000 (6.4e-05, 6.4e-05) x4 nb1 1x32x32                     | 9.3e-08 (8.2e-08) x4 nb1 1x96x128
  b0.d2      all          |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 8.9e-08 (7.8e-08) x4 nb1 2x72x24
  b0.d2      img_border   |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 8.7e-08 (7.8e-08) x4 nb1 2x72x24
  b0.d2      cover1       |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 8.8e-08 (7.8e-08) x4 nb1 2x72x24
  b0.d2      cover2       |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 9.0e-08 (7.9e-08) x4 nb1 2x72x24
  b0.d2      cover4       |  1.000 (2.5e-03, 2.5e-03) x4 nb1 1x32x32                     | 9.7e-08 (8.3e-08) x4 nb1 2x72x24
  b0.d2      image        |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 8.9e-08 (7.8e-08) x4 nb1 2x72x24
  b0.d2      chan_mean    |  1.000 (1.3e-04, 1.3e-04) x4 nb1 1x32x32                     | 5.1e-08 (4.9e-08) x4 nb1 2x72x24
  b0.d3      all          |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 1.2e-07 (1.4e-07) x4 nb1 2x72x24
  b0.d3      img_border   |  1.000 (2.4e-03, 2.4e-03) x4 nb1 1x32x32                     | 1.2e-07 (1.4e-07) x4 nb1 2x72x24
  b0.d3      cover1       |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 1.2e-07 (1.1e-07) x4 nb1 1x32x32
  b0.d3      image        |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 1.3e-07 (1.5e-07) x4 nb1 2x72x24
  b0.d3      chan_mean    |  1.000 (3.0e-04, 3.0e-04) x4 nb1 1x32x32                     | 8.2e-08 (6.4e-08) x4 nb1 1x32x32
  b0.qkv3    all          |  1.000 (5.0e-03, 5.0e-03) x4 nb1 1x32x32                     | 4.1e-07 (2.9e-07) x4 nb1 1x32x32
  b0.qkv3    img_border   |  1.000 (5.4e-03, 5.4e-03) x4 nb1 2x40x56                     | 4.2e-07 (4.1e-07) x4 nb1 3x64x96
  b0.qkv3    cover1       |  1.000 (4.7e-03, 4.7e-03) x4 nb1 1x32x32                     | 4.2e-07 (4.1e-07) x4 nb1 2x72x24
  b0.qkv3    image        |  1.000 (5.0e-03, 5.0e-03) x4 nb1 1x32x32                     | 4.1e-07 (2.9e-07) x4 nb1 1x32x32
  b0.qkv3    chan_mean    |  1.001 (1.3e-04, 1.3e-04) x4 nb1 2x72x24                     | 5.1e-08 (3.5e-08) x4 nb1 1x32x32
  b0.d4      all          |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 1.4e-07 (1.1e-07) x4 nb1 2x72x24
  b0.d4      img_border   |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 1.4e-07 (1.1e-07) x4 nb1 1x96x128
  b0.d4      cover1       |  1.000 (2.4e-03, 2.4e-03) x4 nb1 1x32x32                     | 1.4e-07 (1.1e-07) x4 nb1 2x72x24
  b0.d4      image        |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 1.4e-07 (1.1e-07) x4 nb1 2x72x24
  b0.d4      chan_mean    |  1.000 (2.6e-04, 2.6e-04) x4 nb1 1x32x32                     | 1.0e-07 (6.5e-08) x4 nb1 1x96x128
  b0.qkv4    all          |  1.000 (5.3e-03, 5.3e-03) x4 nb1 1x32x32                     | 4.1e-07 (4.0e-07) x4 nb1 1x96x128
  b0.qkv4    img_border   |  1.000 (5.2e-03, 5.2e-03) x4 nb1 1x32x32                     | 4.1e-07 (4.0e-07) x4 nb1 3x64x96
  b0.qkv4    cover1       |  1.000 (5.4e-03, 5.4e-03) x4 nb1 1x32x32                     | 4.0e-07 (4.0e-07) x4 nb1 1x96x128
  b0.qkv4    image        |  1.000 (5.3e-03, 5.3e-03) x4 nb1 1x32x32                     | 4.1e-07 (4.0e-07) x4 nb1 2x40x56
  b0.qkv4    chan_mean    |  1.004 (2.1e-04, 2.1e-04) x4 nb1 1x32x32                     | 4.8e-08 (3.3e-08) x4 nb1 1x32x32
  b0.xc[1]   all          |  1.000 (2.5e-03, 2.5e-03) x4 nb1 1x32x32                     | 1.2e-07 (9.9e-08) x4 nb1 1x96x128
  b0.xc[1]   win_corner   |  1.000 (2.5e-03, 2.5e-03) x4 nb1 1x32x32                     | 1.2e-07 (9.8e-08) x4 nb1 1x96x128
  b0.xc[1]   win_edge     |  1.000 (2.4e-03, 2.4e-03) x4 nb1 2x72x24                     | 1.2e-07 (1.0e-07) x4 nb1 1x96x128
  b0.xc[1]   win_interior |  1.000 (2.4e-03, 2.4e-03) x4 nb1 1x32x32                     | 1.1e-07 (9.8e-08) x4 nb1 1x96x128
  b0.xc[1]   image        |  1.000 (2.5e-03, 2.5e-03) x4 nb1 1x32x32                     | 1.2e-07 (9.9e-08) x4 nb1 1x96x128
  b0.xc[1]   chan_mean    |  1.003 (7.1e-05, 7.1e-05) x4 nb1 2x72x24 plain               | 9.3e-08 (8.1e-08) x4 nb1 1x96x128
  b0.xc[2]   all          |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 8.3e-08 (7.3e-08) x4 nb1 2x72x24
  b0.xc[2]   win_corner   |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 8.3e-08 (7.4e-08) x4 nb1 2x72x24
  b0.xc[2]   image        |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 8.3e-08 (7.2e-08) x4 nb1 2x72x24
  b0.xc[2]   chan_mean    |  1.007 (2.4e-05, 2.4e-05) x4 nb1 1x96x128                    | 5.0e-08 (4.9e-08) x4 nb1 2x72x24
  b0.xc[3]   all          |  1.000 (2.1e-03, 2.1e-03) x4 nb1 1x32x32                     | 1.1e-07 (1.3e-07) x4 nb1 2x72x24
  b0.xc[3]   win_corner   |  1.000 (2.1e-03, 2.1e-03) x4 nb1 1x32x32                     | 1.1e-07 (1.3e-07) x4 nb1 2x72x24
  b0.xc[3]   image        |  1.000 (2.1e-03, 2.1e-03) x4 nb1 1x32x32                     | 1.2e-07 (1.4e-07) x4 nb1 2x72x24
  b0.xc[3]   chan_mean    |  1.001 (4.2e-05, 4.2e-05) x4 nb1 2x40x56                     | 8.2e-08 (6.4e-08) x4 nb1 1x32x32
  b0.xc[4]   all          |  1.000 (2.1e-03, 2.1e-03) x4 nb1 1x32x32                     | 1.3e-07 (9.9e-08) x4 nb1 2x72x24
  b0.xc[4]   win_corner   |  1.000 (2.1e-03, 2.1e-03) x4 nb1 1x32x32                     | 1.3e-07 (1.0e-07) x4 nb1 2x72x24
  b0.xc[4]   image        |  1.000 (2.1e-03, 2.1e-03) x4 nb1 1x32x32                     | 1.3e-07 (1.0e-07) x4 nb1 2x72x24
  b0.xc[4]   chan_mean    |  1.002 (3.3e-05, 3.3e-05) x4 nb1 2x40x56                     | 1.0e-07 (6.5e-08) x4 nb1 1x96x128
  X1         all          |  1.000 (2.5e-03, 2.5e-03) x4 nb1 1x32x32                     | 1.5e-07 (1.4e-07) x4 nb2 2x40x56
  X1         border       |  1.000 (2.3e-03, 2.3e-03) x4 nb1 1x32x32                     | 1.1e-07 (9.9e-08) x4 nb2 2x40x56
  X1         interior     |  1.000 (2.5e-03, 2.5e-03) x4 nb1 1x32x32                     | 1.5e-07 (1.4e-07) x4 nb2 2x40x56
  X1         chan_mean    |  1.000 (6.0e-05, 6.0e-05) x4 nb1 1x32x32                     | 2.3e-09 (2.2e-09) x4 nb1 1x32x32
  t1act      all          |  1.000 (2.5e-03, 2.5e-03) x4 nb1 1x32x32                     | 1.9e-07 (1.5e-07) x3 nb1 2x72x24
  t1act      border       |  1.000 (2.6e-03, 2.6e-03) x4 nb1 1x32x32                     | 1.9e-07 (1.5e-07) x4 nb1 1x32x32
  t1act      interior     |  1.000 (2.5e-03, 2.5e-03) x4 nb1 1x32x32                     | 1.9e-07 (1.5e-07) x3 nb1 2x72x24
  t1act      chan_mean    |  1.000 (7.6e-04, 7.6e-04) x4 nb1 1x32x32                     | 6.8e-08 (1.2e-09) x4 nb1 2x72x24
  t1der      all          |  1.000 (1.7e-03, 1.7e-03) x4 nb1 1x32x32                     | 1.3e-07 (6.3e-08) x4 nb1 1x32x32
  t1der      border       |  1.000 (1.8e-03, 1.8e-03) x4 nb1 1x32x32                     | 1.3e-07 (6.3e-08) x4 nb1 1x32x32
  t1der      interior     |  1.000 (1.7e-03, 1.7e-03) x4 nb1 1x32x32                     | 1.3e-07 (6.3e-08) x4 nb1 3x64x96
  t1der      chan_mean    |  1.000 (3.6e-04, 3.6e-04) x4 nb1 2x72x24                     | 3.6e-08 (9.3e-10) x4 nb2 2x40x56
  t2act      all          |  1.000 (5.3e-03, 5.3e-03) x4 nb1 1x32x32                     | 3.0e-07 (2.2e-07) x4 nb1 1x32x32
  t2act      border       |  1.000 (5.4e-03, 5.4e-03) x4 nb1 1x32x32                     | 3.1e-07 (2.3e-07) x4 nb1 1x32x32
  t2act      interior     |  1.000 (5.3e-03, 5.3e-03) x4 nb1 1x32x32                     | 3.0e-07 (2.2e-07) x4 nb1 1x32x32
  t2act      chan_mean    |  1.000 (1.1e-03, 1.1e-03) x4 nb1 1x32x32                     | 7.7e-08 (1.4e-09) x4 nb2 2x40x56
  t2der      all          |  1.000 (1.9e-03, 1.9e-03) x4 nb1 1x32x32                     | 1.7e-07 (4.7e-08) x4 nb1 3x64x96
  t2der      border       |  1.000 (1.9e-03, 1.9e-03) x4 nb1 1x32x32                     | 1.7e-07 (4.7e-08) x4 nb1 1x32x32
  t2der      interior     |  1.001 (1.9e-03, 1.9e-03) x4 nb1 1x96x128                    | 1.7e-07 (4.7e-08) x4 nb1 3x64x96
  t2der      chan_mean    |  1.000 (1.3e-04, 1.3e-04) x4 nb1 1x32x32                     | 4.0e-08 (3.0e-10) x4 nb2 2x40x56
  srpre      all          |  1.000 (7.0e-04, 7.0e-04) x4 nb1 1x32x32                     | 9.6e-07 (1.1e-06) x2 nb1 2x40x56
  srpre      border       |  1.000 (1.8e-03, 1.8e-03) x4 nb1 1x32x32                     | 9.6e-07 (1.1e-06) x2 nb1 2x40x56
  srpre      interior     |  1.000 (6.9e-04, 6.9e-04) x4 nb1 1x32x32                     | 9.6e-07 (1.1e-06) x2 nb1 2x40x56
  srpre      crop         |  1.000 (7.0e-04, 7.0e-04) x4 nb1 1x32x32                     | 9.6e-07 (1.1e-06) x2 nb1 2x72x24
  srpre      chan_mean    |  1.000 (7.7e-05, 7.7e-05) x4 nb1 1x32x32                     | 1.0e-08 (1.1e-08) x2 nb1 2x72x24
  sr         all          |  0.000 (0.0e+00, 0.0e+00) x4 nb1 1x32x32                     | 0.0e+00 (0.0e+00) x4 nb1 1x32x32
  X0         pad          |  1.000 (1.7e-03, 1.7e-03) x4 nb1 2x40x56                     | 1.2e-07 (2.4e-07) x4 nb1 2x72x24
  b0.d1      pad          |  1.000 (1.7e-03, 1.7e-03) x4 nb1 2x40x56                     | 1.2e-07 (1.1e-07) x4 nb1 2x40x56
  b0.d2      pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb1 2x40x56                     | 8.8e-08 (7.8e-08) x4 nb1 2x72x24
  b0.d3      cover2       |  1.000 (2.3e-03, 2.3e-03) x4 nb1 2x40x56                     | 1.3e-07 (1.4e-07) x4 nb1 2x72x24
  b0.d3      cover4       |  1.000 (2.3e-03, 2.3e-03) x4 nb1 2x40x56                     | 1.2e-07 (1.5e-07) x4 nb1 1x96x128
  b0.d3      pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb1 2x40x56                     | 1.2e-07 (1.4e-07) x4 nb1 2x72x24
  b0.qkv3    cover2       |  1.000 (5.6e-03, 5.6e-03) x4 nb1 2x40x56                     | 4.1e-07 (4.1e-07) x4 nb1 2x40x56
  b0.qkv3    cover4       |  1.000 (5.1e-03, 5.1e-03) x4 nb1 2x40x56                     | 4.2e-07 (4.1e-07) x4 nb1 2x40x56
  b0.qkv3    pad          |  1.000 (6.0e-03, 6.0e-03) x4 nb1 2x40x56                     | 4.2e-07 (4.1e-07) x4 nb1 2x72x24
  b0.d4      cover2       |  1.000 (2.4e-03, 2.4e-03) x4 nb1 2x40x56                     | 1.4e-07 (1.1e-07) x4 nb1 1x96x128
  b0.d4      cover4       |  1.000 (2.3e-03, 2.3e-03) x4 nb1 3x64x96                     | 1.4e-07 (1.1e-07) x4 nb1 1x96x128
  b0.d4      pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb1 2x40x56                     | 1.3e-07 (1.1e-07) x4 nb1 2x72x24
  b0.qkv4    cover2       |  1.000 (5.8e-03, 5.8e-03) x4 nb1 2x40x56                     | 4.1e-07 (4.0e-07) x4 nb1 1x96x128
  b0.qkv4    cover4       |  1.000 (5.9e-03, 5.9e-03) x4 nb1 2x40x56                     | 4.1e-07 (4.0e-07) x4 nb1 2x40x56
  b0.qkv4    pad          |  1.000 (5.1e-03, 5.1e-03) x4 nb1 2x40x56                     | 4.0e-07 (4.0e-07) x4 nb1 2x72x24
  b0.xc[1]   pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb1 2x40x56                     | 1.3e-07 (1.2e-07) x4 nb1 2x40x56
  b0.xc[2]   win_edge     |  1.000 (2.3e-03, 2.3e-03) x4 nb1 2x40x56                     | 8.3e-08 (7.2e-08) x4 nb1 2x72x24
  b0.xc[2]   win_interior |  1.000 (2.3e-03, 2.3e-03) x4 nb1 2x40x56                     | 7.0e-08 (7.1e-08) x4 nb1 1x96x128
  b0.xc[2]   pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb1 2x40x56                     | 8.3e-08 (7.3e-08) x4 nb1 2x72x24
  b0.xc[3]   pad          |  1.000 (2.2e-03, 2.2e-03) x4 nb1 2x40x56                     | 1.1e-07 (1.3e-07) x4 nb1 2x72x24
  b0.xc[4]   pad          |  1.000 (2.2e-03, 2.2e-03) x4 nb1 2x40x56                     | 1.2e-07 (9.8e-08) x4 nb1 2x72x24
  srpre      outside      |  1.000 (7.0e-04, 7.0e-04) x4 nb1 2x40x56                     | 9.6e-07 (1.1e-06) x2 nb1 2x40x56
  b0.xc[3]   win_edge     |  1.000 (2.2e-03, 2.2e-03) x4 nb1 3x64x96                     | 1.1e-07 (1.3e-07) x4 nb1 2x72x24
  b0.xc[4]   win_edge     |  1.000 (2.2e-03, 2.2e-03) x4 nb1 3x64x96                     | 1.3e-07 (9.7e-08) x4 nb1 1x96x128
  b0.xc[3]   win_interior |  1.000 (2.2e-03, 2.2e-03) x4 nb1 1x96x128                    | 1.1e-07 (1.3e-07) x4 nb1 1x96x128
  b0.xc[4]   win_interior |  1.000 (2.2e-03, 2.2e-03) x4 nb1 1x96x128                    | 1.3e-07 (9.6e-08) x4 nb1 1x96x128
  b1.mean    all          |  0.761 (3.1e-08, 4.0e-08) x4 nb2 2x40x56                     | 4.1e-08 (5.2e-08) x4 nb2 2x40x56
  b1.rstd    all          |  1.199 (5.2e-08, 4.3e-08) x4 nb2 2x40x56                     | 4.9e-08 (4.0e-08) x4 nb2 2x40x56
  b1.d1      all          |  1.000 (1.7e-03, 1.7e-03) x4 nb2 2x40x56                     | 8.4e-08 (1.0e-07) x4 nb2 2x40x56
  b1.d1      img_border   |  1.000 (1.7e-03, 1.7e-03) x4 nb2 2x40x56                     | 8.4e-08 (1.0e-07) x4 nb2 2x40x56
  b1.d1      cover1       |  1.000 (1.7e-03, 1.7e-03) x4 nb2 2x40x56                     | 8.4e-08 (1.0e-07) x4 nb2 2x40x56
  b1.d1      cover2       |  1.000 (1.6e-03, 1.6e-03) x4 nb2 2x40x56                     | 8.3e-08 (1.0e-07) x4 nb2 2x40x56
  b1.d1      cover4       |  1.000 (1.7e-03, 1.7e-03) x4 nb2 2x40x56                     | 8.4e-08 (1.0e-07) x4 nb2 2x40x56
  b1.d1      pad          |  1.000 (1.7e-03, 1.7e-03) x4 nb2 2x40x56                     | 9.0e-08 (1.2e-07) x4 nb2 2x40x56
  b1.d1      image        |  1.000 (1.7e-03, 1.7e-03) x4 nb2 2x40x56                     | 8.0e-08 (9.5e-08) x4 nb2 2x40x56
  b1.d1      chan_mean    |  1.003 (5.5e-05, 5.4e-05) x4 nb2 2x40x56                     | 5.5e-08 (8.6e-08) x4 nb2 2x40x56
  b1.d2      all          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 7.4e-08 (8.5e-08) x4 nb2 2x40x56
  b1.d2      img_border   |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 7.4e-08 (8.5e-08) x4 nb2 2x40x56
  b1.d2      cover1       |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 7.4e-08 (8.5e-08) x4 nb2 2x40x56
  b1.d2      cover2       |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 7.4e-08 (8.5e-08) x4 nb2 2x40x56
  b1.d2      cover4       |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 7.7e-08 (8.9e-08) x4 nb2 2x40x56
  b1.d2      pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 7.9e-08 (9.3e-08) x4 nb2 2x40x56
  b1.d2      image        |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 7.1e-08 (8.1e-08) x4 nb2 2x40x56
  b1.d2      chan_mean    |  1.000 (8.0e-05, 8.0e-05) x4 nb2 2x40x56                     | 4.3e-08 (6.2e-08) x4 nb2 2x40x56
  b1.d3      all          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.0e-07 (1.1e-07) x4 nb2 2x40x56
  b1.d3      img_border   |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.0e-07 (1.1e-07) x4 nb2 2x40x56
  b1.d3      cover1       |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.1e-07 (1.1e-07) x4 nb2 2x40x56
  b1.d3      cover2       |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 9.9e-08 (1.1e-07) x4 nb2 2x40x56
  b1.d3      cover4       |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.d3      pad          |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.d3      image        |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.0e-07 (1.1e-07) x4 nb2 2x40x56
  b1.d3      chan_mean    |  1.000 (1.5e-04, 1.5e-04) x4 nb2 2x40x56                     | 6.2e-08 (7.7e-08) x4 nb2 2x40x56
  b1.qkv3    all          |  1.000 (4.4e-03, 4.4e-03) x4 nb2 2x40x56                     | 3.9e-07 (3.8e-07) x4 nb2 2x40x56
  b1.qkv3    img_border   |  1.000 (4.0e-03, 4.0e-03) x4 nb2 2x40x56                     | 3.7e-07 (3.7e-07) x4 nb2 2x40x56
  b1.qkv3    cover1       |  1.000 (4.5e-03, 4.5e-03) x4 nb2 2x40x56                     | 3.9e-07 (3.9e-07) x4 nb2 2x40x56
  b1.qkv3    cover2       |  1.000 (4.8e-03, 4.8e-03) x4 nb2 2x40x56                     | 4.0e-07 (3.9e-07) x4 nb2 2x40x56
  b1.qkv3    cover4       |  1.000 (3.8e-03, 3.8e-03) x4 nb2 2x40x56                     | 3.9e-07 (3.8e-07) x4 nb2 2x40x56
  b1.qkv3    pad          |  1.000 (4.4e-03, 4.4e-03) x4 nb2 2x40x56                     | 3.7e-07 (3.7e-07) x4 nb2 2x40x56
  b1.qkv3    image        |  1.000 (4.5e-03, 4.5e-03) x4 nb2 2x40x56                     | 3.9e-07 (3.9e-07) x4 nb2 2x40x56
  b1.qkv3    chan_mean    |  1.000 (1.1e-04, 1.1e-04) x4 nb2 2x40x56                     | 2.4e-08 (2.3e-08) x4 nb2 2x40x56
  b1.d4      all          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.4e-07 (1.5e-07) x4 nb2 2x40x56
  b1.d4      img_border   |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.4e-07 (1.5e-07) x4 nb2 2x40x56
  b1.d4      cover1       |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.4e-07 (1.5e-07) x4 nb2 2x40x56
  b1.d4      cover2       |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.3e-07 (1.4e-07) x4 nb2 2x40x56
  b1.d4      cover4       |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.4e-07 (1.5e-07) x4 nb2 2x40x56
  b1.d4      pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.4e-07 (1.6e-07) x4 nb2 2x40x56
  b1.d4      image        |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.3e-07 (1.4e-07) x4 nb2 2x40x56
  b1.d4      chan_mean    |  1.000 (1.5e-04, 1.5e-04) x4 nb2 2x40x56                     | 9.9e-08 (1.2e-07) x4 nb2 2x40x56
  b1.qkv4    all          |  1.000 (3.7e-03, 3.7e-03) x4 nb2 2x40x56                     | 3.7e-07 (3.7e-07) x4 nb2 2x40x56
  b1.qkv4    img_border   |  1.000 (3.4e-03, 3.4e-03) x4 nb2 2x40x56                     | 3.6e-07 (3.5e-07) x4 nb2 2x40x56
  b1.qkv4    cover1       |  1.000 (3.8e-03, 3.8e-03) x4 nb2 2x40x56                     | 3.7e-07 (3.7e-07) x4 nb2 2x40x56
  b1.qkv4    cover2       |  1.000 (4.0e-03, 4.0e-03) x4 nb2 2x40x56                     | 3.7e-07 (3.7e-07) x4 nb2 2x40x56
  b1.qkv4    cover4       |  1.000 (5.0e-03, 5.0e-03) x4 nb2 2x40x56                     | 3.7e-07 (3.7e-07) x4 nb2 2x40x56
  b1.qkv4    pad          |  1.000 (3.3e-03, 3.3e-03) x4 nb2 2x40x56                     | 3.5e-07 (3.5e-07) x4 nb2 2x40x56
  b1.qkv4    image        |  1.000 (4.1e-03, 4.1e-03) x4 nb2 2x40x56                     | 3.8e-07 (3.8e-07) x4 nb2 2x40x56
  b1.qkv4    chan_mean    |  0.999 (1.1e-04, 1.1e-04) x4 nb2 2x40x56                     | 2.4e-08 (2.4e-08) x4 nb2 2x40x56
  b1.xc[1]   all          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 9.1e-08 (1.1e-07) x4 nb2 2x40x56
  b1.xc[1]   win_corner   |  1.000 (2.5e-03, 2.5e-03) x4 nb2 2x40x56                     | 8.6e-08 (1.0e-07) x4 nb2 2x40x56
  b1.xc[1]   win_edge     |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 9.0e-08 (1.1e-07) x4 nb2 2x40x56
  b1.xc[1]   win_interior |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 9.2e-08 (1.1e-07) x4 nb2 2x40x56
  b1.xc[1]   pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 9.6e-08 (1.2e-07) x4 nb2 2x40x56
  b1.xc[1]   image        |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 8.8e-08 (1.0e-07) x4 nb2 2x40x56
  b1.xc[1]   chan_mean    |  1.003 (6.5e-05, 6.5e-05) x4 nb2 2x40x56                     | 5.5e-08 (8.6e-08) x4 nb2 2x40x56
  b1.xc[2]   all          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 6.8e-08 (8.0e-08) x4 nb2 2x40x56
  b1.xc[2]   win_corner   |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 6.8e-08 (8.0e-08) x4 nb2 2x40x56
  b1.xc[2]   win_edge     |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 6.7e-08 (7.9e-08) x4 nb2 2x40x56
  b1.xc[2]   win_interior |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 6.8e-08 (8.1e-08) x4 nb2 2x40x56
  b1.xc[2]   pad          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 7.2e-08 (8.8e-08) x4 nb2 2x40x56
  b1.xc[2]   image        |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 6.5e-08 (7.6e-08) x4 nb2 2x40x56
  b1.xc[2]   chan_mean    |  1.000 (4.4e-05, 4.4e-05) x4 nb2 2x40x56                     | 4.3e-08 (6.2e-08) x4 nb2 2x40x56
  b1.xc[3]   all          |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 9.0e-08 (1.0e-07) x4 nb2 2x40x56
  b1.xc[3]   win_corner   |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 9.0e-08 (1.0e-07) x4 nb2 2x40x56
  b1.xc[3]   pad          |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 9.2e-08 (1.0e-07) x4 nb2 2x40x56
  b1.xc[3]   image        |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 8.9e-08 (9.8e-08) x4 nb2 2x40x56
  b1.xc[3]   chan_mean    |  0.996 (3.9e-05, 3.9e-05) x4 nb2 2x40x56                     | 6.2e-08 (7.7e-08) x4 nb2 2x40x56
  b1.xc[4]   all          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.2e-07 (1.4e-07) x4 nb2 2x40x56
  b1.xc[4]   win_corner   |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.2e-07 (1.4e-07) x4 nb2 2x40x56
  b1.xc[4]   pad          |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 1.3e-07 (1.5e-07) x4 nb2 2x40x56
  b1.xc[4]   image        |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 1.2e-07 (1.3e-07) x4 nb2 2x40x56
  b1.xc[4]   chan_mean    |  1.000 (3.4e-05, 3.4e-05) x4 nb2 2x40x56                     | 9.8e-08 (1.2e-07) x4 nb2 2x40x56
  X2         all          |  1.000 (2.4e-03, 2.4e-03) x4 nb2 2x40x56                     | 2.1e-07 (9.7e-08) x4 nb2 2x40x56
  X2         border       |  1.000 (2.3e-03, 2.3e-03) x4 nb2 2x40x56                     | 1.6e-07 (7.5e-08) x4 nb2 2x40x56
  X2         interior     |  1.000 (2.5e-03, 2.5e-03) x4 nb2 2x40x56                     | 2.1e-07 (9.8e-08) x4 nb2 2x40x56
  X2         chan_mean    |  1.000 (2.8e-05, 2.8e-05) x4 nb2 2x40x56                     | 3.3e-09 (1.6e-09) x4 nb2 2x40x56
  b0.qkv1    all          |  1.000 (5.5e-03, 5.5e-03) x4 nb1 2x40x56 qkv                 | 1.1e-07 (1.4e-07) x4 nb1 3x64x96
  b0.qkv1    img_border   |  1.000 (5.4e-03, 5.4e-03) x4 nb1 2x40x56 qkv                 | 1.2e-07 (1.4e-07) x4 nb1 1x32x32
  b0.qkv1    cover1       |  1.000 (5.7e-03, 5.7e-03) x4 nb1 2x40x56 qkv                 | 1.1e-07 (1.4e-07) x4 nb1 1x96x128
  b0.qkv1    cover2       |  1.000 (5.3e-03, 5.3e-03) x4 nb1 2x40x56 qkv                 | 1.1e-07 (1.4e-07) x4 nb1 3x64x96
  b0.qkv1    cover4       |  1.000 (4.9e-03, 4.9e-03) x4 nb1 2x40x56 qkv                 | 1.2e-07 (1.5e-07) x4 nb1 1x32x32
  b0.qkv1    image        |  1.000 (5.5e-03, 5.5e-03) x4 nb1 2x40x56 qkv                 | 1.1e-07 (1.4e-07) x4 nb1 3x64x96
  b0.qkv1    chan_mean    |  1.000 (2.1e-05, 2.1e-05) x4 nb1 2x40x56 qkv                 | 3.9e-09 (5.3e-09) x4 nb1 1x32x32
  b0.qkv2    all          |  1.000 (5.6e-03, 5.6e-03) x4 nb1 2x40x56 qkv                 | 2.2e-07 (2.2e-07) x4 nb1 2x40x56
  b0.qkv2    img_border   |  1.000 (5.7e-03, 5.7e-03) x4 nb1 2x40x56 qkv                 | 2.2e-07 (2.2e-07) x4 nb1 3x64x96
  b0.qkv2    cover1       |  1.000 (5.5e-03, 5.5e-03) x4 nb1 2x40x56 qkv                 | 2.2e-07 (2.2e-07) x4 nb1 2x72x24
  b0.qkv2    cover2       |  1.000 (5.6e-03, 5.6e-03) x4 nb1 2x40x56 qkv                 | 2.2e-07 (2.2e-07) x4 nb1 2x40x56
  b0.qkv2    cover4       |  1.000 (5.4e-03, 5.4e-03) x4 nb1 2x40x56 qkv                 | 2.3e-07 (2.2e-07) x4 nb1 1x96x96
  b0.qkv2    image        |  1.000 (5.3e-03, 5.3e-03) x4 nb1 2x40x56 qkv                 | 2.2e-07 (2.2e-07) x4 nb1 2x72x24
  b0.qkv2    chan_mean    |  1.000 (6.4e-05, 6.4e-05) x4 nb1 2x72x24 plain               | 1.2e-08 (1.3e-08) x4 nb1 1x32x32
  b0.qkv1    pad          |  1.000 (5.5e-03, 5.5e-03) x4 nb1 2x40x56 qkv                 | 1.1e-07 (1.4e-07) x4 nb1 2x72x24
  b0.qkv2    pad          |  1.000 (6.3e-03, 6.3e-03) x4 nb1 2x40x56 qkv                 | 2.3e-07 (2.2e-07) x4 nb1 2x40x56
  b1.qkv1    all          |                                                              | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.qkv1    img_border   |                                                              | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.qkv1    cover1       |                                                              | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.qkv1    cover2       |                                                              | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.qkv1    cover4       |                                                              | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.qkv1    pad          |                                                              | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.qkv1    image        |                                                              | 1.1e-07 (1.2e-07) x4 nb2 2x40x56
  b1.qkv1    chan_mean    |                                                              | 1.6e-09 (1.7e-09) x4 nb2 2x40x56
  b1.qkv2    all          |                                                              | 2.2e-07 (2.1e-07) x4 nb2 2x40x56
  b1.qkv2    img_border   |                                                              | 2.0e-07 (2.0e-07) x4 nb2 2x40x56
  b1.qkv2    cover1       |                                                              | 2.2e-07 (2.1e-07) x4 nb2 2x40x56
  b1.qkv2    cover2       |                                                              | 2.3e-07 (2.2e-07) x4 nb2 2x40x56
  b1.qkv2    cover4       |                                                              | 2.2e-07 (2.1e-07) x4 nb2 2x40x56
  b1.qkv2    pad          |                                                              | 2.2e-07 (2.1e-07) x4 nb2 2x40x56
  b1.qkv2    image        |                                                              | 2.2e-07 (2.1e-07) x4 nb2 2x40x56
  b1.qkv2    chan_mean    |                                                              | 6.8e-09 (6.6e-09) x4 nb2 2x40x56
"""
import pytest
import torch

from oracle import m2trans_oracle as O
from tests import fwd_stage_ref as R
from tests.gpu_util import build_model, hip_forward_trace

pytestmark = pytest.mark.gpu

PLAIN = {"fused_attn_fwd": 0, "fused_c16_fwd": 0, "fused_prep_fwd": 0, "conv_rows": 0, "fused_tail": 0}


def _set(plan, key, value):
    from m2trans_amd import _lib
    _lib.check(_lib.load().m2t_set_option(plan.handle, key.encode(), int(value)), "m2t_set_option " + key)


def _forward(model, plan, xd, scale, nb, B, H, W):
    with torch.no_grad():
        sr = model(xd)
    torch.cuda.synchronize()
    return sr.cpu(), hip_forward_trace(plan, scale, nb, B, H, W)


def _assert_common_equal(a, b, what):
    diff = [n for n in a if n in b and not torch.equal(a[n], b[n])]
    assert not diff, f"{what}: {diff} differ"


def _gate(scale, nb, B, H0, W0, dtype, opts=None, same_as_default=False, expect=None):
    """opts: plan options of the gated run; same_as_default: the default run goes first and every tensor both runs store must be bit-equal;
    expect: {query key: value} that must hold under the options (the kernel the cell is about did run)."""
    model, p = build_model(scale, nb, dtype)
    x = O.closed_form_image(B, 3, H0, W0)
    xd = x.cuda()
    plan = model._plan_for(xd)
    H, W = plan.query("padded_h"), plan.query("padded_w")
    assert (H, W) == ((H0 + 31) // 32 * 32, (W0 + 31) // 32 * 32)
    args = (model, plan, xd, scale, nb, B, H, W)
    if same_as_default:
        sr0, trace0 = _forward(*args)
    for k, v in (opts or {}).items():
        _set(plan, k, v)
    for k, v in (expect or {}).items():
        assert plan.query(k) == v, (k, plan.query(k), v)
    extra = {}
    stores, names = ("stores_t2", ("t2act", "t2der")) if scale == 4 else ("stores_t1", ("t1act", "t1der"))
    if plan.query(stores) == 0:
        default = plan.query("opt:fused_tail")
        _set(plan, "fused_tail", 1 if scale == 4 else 0)
        assert plan.query(stores) == 1
        sr_stored, tr_stored = _forward(*args)
        extra = {n: tr_stored[n] for n in names}
        _set(plan, "fused_tail", default)
        assert plan.query(stores) == 0
    sr, taps = _forward(*args)
    if extra:
        assert torch.equal(sr, sr_stored), "the stored-form tail is not bit-identical in the forward pass"
        _assert_common_equal(taps, tr_stored, "stored-form run against the default run")
        taps.update(extra)
    if same_as_default:
        assert torch.equal(sr, sr0), "sr differs from the default run's"
        _assert_common_equal(taps, trace0, f"{opts} against the default run")
    del model
    taps["sr"] = sr
    crop = taps["srpre"][..., :H0 * scale, :W0 * scale]
    assert bool(((crop < 0) | (crop > 1)).any())                 # the clamp is live
    stored_qkv = tuple(i for i in (1, 2, 3, 4) if f"b0.qkv{i}" in taps)
    g = R.geometry(x, p, scale, nb, dtype, stored_qkv=stored_qkv, conv_stats=(dtype == "bf16" and (opts or {}).get("conv_rows", 1) == 1))
    bad, table, _ = R.gate(g, taps)
    print(f"\nx{scale} nb={nb} {B}x{H0}x{W0} {dtype}{' ' + str(opts) if opts else ''}: error, " +
          ("budget, error / budget" if dtype == "bf16" else "float32 oracle's error, ratio"))
    print(R.format_table(table))
    missing = R.required_entries(g) - set(table)
    assert not missing, missing
    assert not bad, "\n".join(bad)
    return g


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,H0,W0", [(1, 32, 32), (2, 40, 56), (3, 64, 96), (1, 96, 128), (1, 96, 96), (2, 72, 24)])
def test_x4_one_block(B, H0, W0, dtype):
    g = _gate(4, 1, B, H0, W0, dtype)
    assert g.stored_qkv == ((3, 4) if dtype == "bf16" else (1, 2, 3, 4))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_x4_two_blocks(dtype):
    """The non-last block, block 1's statistics out of the conv's epilogue (bf16), the X0 fold in the last block only."""
    _gate(4, 2, 2, 40, 56, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,H0,W0", [(2, 40, 56), (2, 72, 24)])
@pytest.mark.parametrize("scale", [2, 3])
def test_x2_x3_one_block(scale, B, H0, W0, dtype):
    """The streaming tails."""
    _gate(scale, 1, B, H0, W0, dtype)


def test_x4_stored_qkv_of_the_fused_forward_kernels():
    """fused_c16_fwd = fused_attn_fwd = 1: the fused kernels store q | k | v of branches 1 and 2, which become stages of their own; every
    other stored tensor is bit-equal to the default (recomputing) run."""
    g = _gate(4, 1, 2, 40, 56, "bf16", opts={"fused_c16_fwd": 1, "fused_attn_fwd": 1}, same_as_default=True,
              expect={"stores_qkv1": 1, "stores_qkv2": 1})
    assert g.stored_qkv == (1, 2, 3, 4)


@pytest.mark.parametrize("B,H0,W0", [(2, 40, 56), (2, 72, 24)])
def test_x4_plain_bf16_forward_kernels(B, H0, W0):
    """branch_prep, gemm_nt, window_attn_fwd with its IWT epilogue, the tile conv, tail_expand x 2 and final_conv_fwd in bf16."""
    g = _gate(4, 1, B, H0, W0, "bf16", opts=PLAIN,
              expect={"opt:fused_attn_fwd": 0, "opt:fused_c16_fwd": 0, "opt:fused_prep_fwd": 0, "opt:conv_rows": 0, "stores_t2": 1})
    assert g.stored_qkv == (1, 2, 3, 4)


@pytest.mark.parametrize("B,H0,W0,variant,in_force", [(3, 64, 96, 1, 1), (3, 64, 96, 2, 2), (1, 96, 96, 2, 1)])
def test_x4_two_windows_per_cu(B, H0, W0, variant, in_force):
    """k_attn_fwd2.hip; at 1x96x96 the 9 level-2 windows are an odd count and variant 2 falls back to one window per workgroup."""
    _gate(4, 1, B, H0, W0, "bf16", opts={"fused_attn_fwd2": variant}, expect={"opt:fused_attn_fwd2": in_force})
