"""-m gpu: teacher-forced stage gate of the backward pass -- every stored gradient of the default schedule against fp64.

The model runs through the autograd surface (lr.requires_grad_(True), loss (sr * w).sum() with a seeded random w, or L1 with part of the
output under the clamp) with DEFAULT plan options: in bf16 mode that is the fused path (the resident attention backward with the
projection data gradient inside it, c16_dgrad_prep, fused_prep_bwd / fused_norm_red, conv3x3_c64_bwd_rows, the fused tail backward).
tests/gpu_util.hip_backward_trace then reads the gradient taps back and tests/bwd_stage_ref.py judges each one against the VJP of the
run's own upstream tap through the float64 oracle (teacher-forced along the run's forward trajectory in bf16 mode), whole tensor and per
pixel class:
  bf16   every entry <= 3 x its budget (the explicit chain with the kernels' bf16 rounding points; lr.grad, an fp32 tensor: the head data
         gradient's 576-term fp32 accumulation chain).  Floor where the budget is exactly zero -- gpre alone: g(sr) times a 0 / 1 mask -- is the
         float32 oracle's own error against float64 on that stage, which is zero too: the seed must be bit-exact, and is;
  fp32   every entry <= 1e-4 of own norm, or <= 3 x the float32 oracle's own error.
Run with -s for each cell's table (error, budget, ratio per (tap, class)).

PARAMETER GRADIENTS.  The same run's q.grad of every model.named_parameters() entry is gated next to the data taps: each against the VJP from
the nearest intact upstream tap to the parameter leaf, with the run's own value of that tap as cotangent (bwd_stage_ref.param_refs),
elementwise in the oracle's shape -- whole tensor and q | k | v row blocks, ring / inner table rows, centre / edge / corner taps,
pixel-unshuffle phases -- so that the deferred reduction's layout modes are judged too.  The cells already sit on the weight-gradient
kernels' edges: 1x32x32 has level-2 M = 64 rows (< 128: generic masked kernel), 2x40x56 M = 512 (fast path), 3x64x96 M = 1152 (9 row blocks
in 5 slabs, the last one partial), C = 16 has N = 48 (generic).  Added: every cell runs its step a second time and requires bit-equal
parameter gradients (the first backward publishes the reduction table and reduces at its end on the side stream, later ones reduce as
they go and run the head's weight gradient on the main stream); one cell forces wgrad_tn_big_kernel; one cell runs the plain bf16
kernels.  The first device run found no kernel fault, two accumulation orders missing from the emulation (the bias gradients of
conv3x3_c64_bwd_rows_kernel and wgrad_tn_kernel: column sums of bf16 values, which a torch float32 sum gets right to 1.4e-8 of own norm
where the kernels' MFMA chains leave 3.4e-8 / 4.8e-8, 2.4x / 3.5x), and that ONE emulation's error of a rel-pos table is too noisy a number
to be a budget (bwd_stage_ref: SCATTER OF THE REL-POS BUDGET): the tables' budget is emulated from the run's own gy.

The gate's first device run found no kernel fault and one point missing from the emulation: with lr.grad's budget taken from the float32
oracle (a blocked sum, 2.3e-7 of own norm at 1x32x32) the head data gradient stood at 3.5x (8.0e-7; 7.2e-7 .. 1.3e-6 in every cell and both
compute types).  head_conv_dgrad_kernel sums its 576 products in one fp32 FMA chain; restated in that order the budget is 4.7e-7 .. 1.2e-6.

MEASURED on MI355X, worst over the cells below per (tap, class): bf16 = error / budget with (error, budget) and the cell; fp32 = error with
(the float32 oracle's own error) and the cell.  Cells are named <scale> nb<blocks> <B>x<H>x<W> [l1].
  tap        class       | bf16: worst error / budget (error, budget), cell          | fp32: worst error (float32 oracle's), cell
  g_t1pre    all         |  1.00 (2.1e-03, 2.1e-03) x4 nb1 1x32x32              | 8.8e-07 (8.5e-07) x4 nb2 2x40x56
  g_t1pre    border      |  1.16 (2.5e-03, 2.2e-03) x4 nb1 1x96x128             | 8.9e-07 (8.9e-07) x4 nb2 2x40x56
  g_t1pre    interior    |  1.00 (2.1e-03, 2.1e-03) x4 nb1 1x32x32              | 8.8e-07 (8.5e-07) x4 nb2 2x40x56
  gT         all         |  1.00 (1.6e-03, 1.6e-03) x4 nb1 1x32x32              | 7.4e-07 (3.7e-07) x4 nb1 2x40x56 l1
  gT         border      |  1.03 (3.3e-03, 3.2e-03) x3 nb1 2x40x56              | 6.5e-07 (7.2e-07) x2 nb1 2x40x56
  gT         interior    |  1.00 (1.6e-03, 1.6e-03) x4 nb1 1x32x32              | 7.6e-07 (3.7e-07) x4 nb1 2x40x56 l1
  b0.gqkv1   all         |  1.01 (4.3e-03, 4.3e-03) x4 nb1 1x32x32              | 1.5e-06 (2.7e-06) x4 nb1 2x40x56
  b0.gqkv1   img_border  |  1.04 (4.6e-03, 4.5e-03) x4 nb1 2x40x56              | 1.3e-06 (2.5e-06) x4 nb1 3x64x96
  b0.gqkv1   cover1      |  1.02 (5.3e-03, 5.3e-03) x4 nb1 2x40x56              | 1.5e-06 (2.9e-06) x4 nb1 2x40x56
  b0.gqkv1   cover2      |  1.02 (4.4e-03, 4.3e-03) x4 nb1 1x32x32              | 1.5e-06 (2.6e-06) x4 nb1 2x40x56
  b0.gqkv1   cover4      |  1.05 (4.5e-03, 4.3e-03) x4 nb1 1x32x32              | 1.7e-06 (3.0e-06) x4 nb1 2x40x56
  b0.gqkv2   all         |  1.03 (7.1e-03, 6.9e-03) x4 nb1 1x32x32              | 2.3e-06 (4.2e-06) x4 nb1 2x40x56
  b0.gqkv2   img_border  |  1.03 (7.0e-03, 6.7e-03) x4 nb1 1x32x32              | 2.2e-06 (4.1e-06) x4 nb1 1x96x128
  b0.gqkv2   cover1      |  1.03 (6.7e-03, 6.5e-03) x4 nb1 1x32x32              | 2.2e-06 (4.0e-06) x4 nb1 2x40x56
  b0.gqkv2   cover2      |  1.02 (7.7e-03, 7.6e-03) x4 nb1 1x32x32              | 2.4e-06 (4.4e-06) x4 nb1 2x40x56
  b0.gqkv2   cover4      |  1.06 (1.2e-02, 1.1e-02) x4 nb1 1x32x32              | 2.7e-06 (4.9e-06) x4 nb1 2x40x56
  b0.gqkv3   all         |  1.01 (2.1e-03, 2.1e-03) x4 nb1 2x40x56 l1           | 1.1e-06 (1.9e-06) x4 nb1 1x32x32
  b0.gqkv3   img_border  |  1.02 (3.2e-03, 3.2e-03) x2 nb1 2x40x56              | 1.1e-06 (1.9e-06) x4 nb1 1x32x32
  b0.gqkv3   cover1      |  1.02 (3.6e-03, 3.5e-03) x3 nb1 2x40x56              | 1.1e-06 (1.9e-06) x4 nb1 1x32x32
  b0.gqkv4   all         |  1.02 (2.6e-03, 2.6e-03) x2 nb1 2x40x56              | 9.0e-07 (1.5e-06) x4 nb1 1x32x32
  b0.gqkv4   img_border  |  1.03 (2.6e-03, 2.5e-03) x2 nb1 2x40x56              | 9.1e-07 (1.5e-06) x4 nb1 1x32x32
  b0.gqkv4   cover1      |  1.02 (2.5e-03, 2.4e-03) x2 nb1 2x40x56              | 9.0e-07 (1.5e-06) x4 nb1 1x32x32
  gn[1]      all         |  1.00 (3.5e-03, 3.5e-03) x4 nb1 1x32x32              | 1.0e-06 (3.8e-06) x4 nb1 2x40x56 l1
  gn[1]      img_border  |  1.03 (3.7e-03, 3.6e-03) x4 nb1 2x40x56              | 1.0e-06 (1.7e-06) x4 nb1 2x40x56
  gn[1]      cover1      |  1.00 (3.5e-03, 3.5e-03) x4 nb1 1x32x32              | 1.1e-06 (4.1e-06) x4 nb1 2x40x56 l1
  gn[1]      cover2      |  1.01 (3.6e-03, 3.6e-03) x4 nb1 1x32x32              | 1.0e-06 (1.0e-06) x3 nb1 2x40x56
  gn[1]      cover4      |  1.01 (3.7e-03, 3.6e-03) x4 nb1 2x40x56              | 1.0e-06 (9.8e-07) x3 nb1 2x40x56
  gn[2]      all         |  1.01 (3.8e-03, 3.7e-03) x4 nb1 1x32x32              | 1.3e-06 (4.8e-06) x4 nb1 2x40x56 l1
  gn[2]      img_border  |  1.06 (3.8e-03, 3.6e-03) x4 nb1 1x32x32              | 1.2e-06 (3.5e-06) x4 nb1 2x40x56 l1
  gn[2]      cover1      |  1.00 (3.8e-03, 3.8e-03) x4 nb1 1x32x32              | 1.3e-06 (4.8e-06) x4 nb1 2x40x56 l1
  gn[2]      cover2      |  1.01 (3.8e-03, 3.8e-03) x4 nb1 1x32x32              | 1.3e-06 (5.1e-06) x4 nb1 2x40x56 l1
  gn[2]      cover4      |  1.02 (4.1e-03, 4.0e-03) x4 nb1 1x32x32              | 1.3e-06 (4.4e-06) x4 nb1 2x40x56 l1
  gn[3]      all         |  1.00 (3.2e-03, 3.2e-03) x4 nb1 2x40x56              | 1.0e-06 (3.7e-06) x4 nb1 2x40x56 l1
  gn[3]      img_border  |  1.01 (3.2e-03, 3.2e-03) x4 nb1 1x96x128             | 1.0e-06 (3.4e-06) x4 nb1 2x40x56 l1
  gn[3]      cover1      |  1.00 (3.2e-03, 3.2e-03) x4 nb1 1x32x32              | 9.9e-07 (3.6e-06) x4 nb1 2x40x56 l1
  gn[4]      all         |  1.00 (2.4e-03, 2.4e-03) x4 nb1 2x40x56              | 7.6e-07 (2.8e-06) x4 nb1 2x40x56 l1
  gn[4]      img_border  |  1.01 (2.4e-03, 2.4e-03) x3 nb1 2x40x56              | 7.4e-07 (2.5e-06) x4 nb1 2x40x56 l1
  gn[4]      cover1      |  1.00 (2.3e-03, 2.4e-03) x4 nb1 2x40x56              | 7.6e-07 (2.9e-06) x4 nb1 2x40x56 l1
  gres       all         |  1.00 (2.2e-03, 2.2e-03) x4 nb1 1x32x32              | 4.4e-08 (4.3e-08) x4 nb2 2x40x56
  gres       border      |  1.02 (2.2e-03, 2.1e-03) x4 nb1 1x32x32              | 4.0e-08 (3.9e-08) x4 nb2 2x40x56
  gres       interior    |  1.00 (2.2e-03, 2.2e-03) x4 nb1 1x32x32              | 4.4e-08 (4.3e-08) x4 nb2 2x40x56
  gres       chan_mean   |  1.07 (3.0e-03, 2.8e-03) x4 nb2 2x40x56              | 3.3e-07 (3.5e-07) x4 nb1 2x40x56
  gres       along_xhat  |  1.04 (1.6e-03, 1.5e-03) x4 nb1 1x96x128             | 1.6e-07 (2.3e-07) x4 nb2 2x40x56
  lr.grad    all         |  1.54 (7.2e-07, 4.7e-07) x2 nb1 2x40x56              | 1.3e-06 (9.0e-07) x4 nb1 2x40x56 l1
  lr.grad    folded      |  1.70 (8.2e-07, 4.8e-07) x4 nb2 2x40x56              | 1.3e-06 (9.1e-07) x4 nb1 2x40x56 l1
  lr.grad    unfolded    |  1.00 (7.7e-07, 7.7e-07) x4 nb1 1x32x32              | 1.2e-06 (8.8e-07) x4 nb1 2x40x56 l1
  lr.grad    border      |  1.34 (5.6e-07, 4.2e-07) x2 nb1 2x40x56              | 9.5e-07 (5.9e-07) x4 nb1 2x40x56 l1
  lr.grad    interior    |  1.55 (7.3e-07, 4.7e-07) x2 nb1 2x40x56              | 1.3e-06 (9.3e-07) x4 nb1 2x40x56 l1
  gpre       all         |  0.00 (0.0e+00, 0.0e+00) x4 nb1 1x32x32              | 0.0e+00 (0.0e+00) x4 nb1 1x32x32
  b0.gqkv3   cover2      |  1.01 (2.3e-03, 2.3e-03) x4 nb1 2x40x56 l1           | 9.3e-07 (9.2e-07) x3 nb1 2x40x56
  b0.gqkv3   cover4      |  1.05 (3.1e-03, 3.0e-03) x2 nb1 2x40x56              | 9.9e-07 (1.8e-06) x4 nb1 1x96x128
  b0.gqkv4   cover2      |  1.02 (3.3e-03, 3.2e-03) x4 nb1 2x40x56              | 7.4e-07 (1.4e-06) x4 nb1 1x96x128
  b0.gqkv4   cover4      |  1.06 (2.7e-03, 2.6e-03) x2 nb1 2x40x56              | 8.0e-07 (1.5e-06) x4 nb1 1x96x128
  gn[3]      cover2      |  1.00 (3.2e-03, 3.2e-03) x4 nb1 2x40x56              | 1.0e-06 (3.8e-06) x4 nb1 2x40x56 l1
  gn[3]      cover4      |  1.03 (3.3e-03, 3.2e-03) x3 nb1 2x40x56              | 1.1e-06 (3.5e-06) x4 nb1 2x40x56 l1
  gn[4]      cover2      |  1.00 (2.4e-03, 2.4e-03) x4 nb1 2x40x56              | 7.6e-07 (3.0e-06) x4 nb1 2x40x56 l1
  gn[4]      cover4      |  1.01 (2.4e-03, 2.4e-03) x4 nb1 2x40x56              | 8.4e-07 (2.6e-06) x4 nb1 2x40x56 l1
  b1.gqkv1   all         |  1.00 (4.4e-03, 4.4e-03) x4 nb2 2x40x56              | 1.1e-06 (1.1e-06) x4 nb2 2x40x56
  b1.gqkv1   img_border  |  0.99 (4.1e-03, 4.2e-03) x4 nb2 2x40x56              | 1.0e-06 (1.2e-06) x4 nb2 2x40x56
  b1.gqkv1   cover1      |  1.00 (4.3e-03, 4.3e-03) x4 nb2 2x40x56              | 1.0e-06 (1.0e-06) x4 nb2 2x40x56
  b1.gqkv1   cover2      |  1.00 (4.5e-03, 4.5e-03) x4 nb2 2x40x56              | 1.1e-06 (1.1e-06) x4 nb2 2x40x56
  b1.gqkv1   cover4      |  0.98 (4.7e-03, 4.8e-03) x4 nb2 2x40x56              | 1.1e-06 (1.2e-06) x4 nb2 2x40x56
  b1.gqkv2   all         |  1.00 (5.2e-03, 5.2e-03) x4 nb2 2x40x56              | 1.3e-06 (1.7e-06) x4 nb2 2x40x56
  b1.gqkv2   img_border  |  0.99 (4.9e-03, 5.0e-03) x4 nb2 2x40x56              | 1.3e-06 (1.7e-06) x4 nb2 2x40x56
  b1.gqkv2   cover1      |  1.01 (4.7e-03, 4.6e-03) x4 nb2 2x40x56              | 1.2e-06 (1.6e-06) x4 nb2 2x40x56
  b1.gqkv2   cover2      |  1.00 (5.7e-03, 5.6e-03) x4 nb2 2x40x56              | 1.4e-06 (1.8e-06) x4 nb2 2x40x56
  b1.gqkv2   cover4      |  1.00 (6.1e-03, 6.0e-03) x4 nb2 2x40x56              | 1.3e-06 (1.7e-06) x4 nb2 2x40x56
  b1.gqkv3   all         |  1.01 (3.6e-03, 3.6e-03) x4 nb2 2x40x56              | 1.2e-06 (1.9e-06) x4 nb2 2x40x56
  b1.gqkv3   img_border  |  1.02 (3.5e-03, 3.5e-03) x4 nb2 2x40x56              | 1.4e-06 (2.1e-06) x4 nb2 2x40x56
  b1.gqkv3   cover1      |  1.01 (3.4e-03, 3.4e-03) x4 nb2 2x40x56              | 1.2e-06 (1.9e-06) x4 nb2 2x40x56
  b1.gqkv3   cover2      |  1.00 (3.8e-03, 3.8e-03) x4 nb2 2x40x56              | 1.1e-06 (1.8e-06) x4 nb2 2x40x56
  b1.gqkv3   cover4      |  1.01 (3.6e-03, 3.6e-03) x4 nb2 2x40x56              | 8.8e-07 (1.5e-06) x4 nb2 2x40x56
  b1.gqkv4   all         |  0.99 (3.0e-03, 3.0e-03) x4 nb2 2x40x56              | 1.2e-06 (1.9e-06) x4 nb2 2x40x56
  b1.gqkv4   img_border  |  0.99 (3.0e-03, 3.0e-03) x4 nb2 2x40x56              | 1.2e-06 (2.1e-06) x4 nb2 2x40x56
  b1.gqkv4   cover1      |  0.99 (2.8e-03, 2.9e-03) x4 nb2 2x40x56              | 1.3e-06 (1.9e-06) x4 nb2 2x40x56
  b1.gqkv4   cover2      |  0.99 (3.3e-03, 3.3e-03) x4 nb2 2x40x56              | 1.1e-06 (1.7e-06) x4 nb2 2x40x56
  b1.gqkv4   cover4      |  0.96 (3.1e-03, 3.3e-03) x4 nb2 2x40x56              | 8.8e-07 (1.1e-06) x4 nb2 2x40x56
  gB         all         |  1.00 (2.5e-03, 2.5e-03) x4 nb2 2x40x56              | 3.5e-07 (1.9e-07) x4 nb2 2x40x56
  gB         border      |  1.00 (2.3e-03, 2.4e-03) x4 nb2 2x40x56              | 2.8e-07 (1.7e-07) x4 nb2 2x40x56
  gB         interior    |  1.00 (2.6e-03, 2.6e-03) x4 nb2 2x40x56              | 3.6e-07 (1.9e-07) x4 nb2 2x40x56
PARAMETER GRADIENTS, MEASURED on MI355X, the same columns; cells as above plus "big" (wgrad_big_tiles = 256) and "plain" (attn_bwd = 0,
fused_conv_bwd = 0, fused_tail = 0: weights and biases only).  ff = feed_forward.0, wqkv = qkv_conv.weight.  A bias whose float32 budget is
a fraction of an ulp shows ratios that mean nothing beyond "both are exact to rounding" (head.bias 2.24 = 9.5e-9 / 4.3e-9).
  parameter           class  | bf16: worst error / budget (error, budget), cell      | fp32: worst error (float32 oracle's), cell
  tail.6.weight       all    |  1.04 (1.2e-03, 1.2e-03) x4 nb1 1x32x32          | 6.3e-07 (1.6e-06) x4 nb2 2x40x56
  tail.6.weight       centre |  1.00 (1.1e-03, 1.1e-03) x4 nb1 1x32x32          | 7.3e-07 (1.6e-06) x4 nb2 2x40x56
  tail.6.weight       edge   |  1.05 (1.3e-03, 1.2e-03) x4 nb1 1x32x32          | 6.5e-07 (1.7e-06) x4 nb2 2x40x56
  tail.6.weight       corner |  1.05 (9.1e-04, 8.7e-04) x4 nb1 1x96x128         | 5.8e-07 (1.6e-06) x4 nb2 2x40x56
  tail.3.weight       all    |  1.05 (3.0e-03, 2.8e-03) x4 nb1 1x32x32          | 1.2e-06 (1.7e-06) x4 nb1 3x64x96
  tail.3.weight       phase0 |  1.04 (2.7e-03, 2.6e-03) x4 nb1 1x32x32          | 1.1e-06 (1.7e-06) x4 nb1 3x64x96
  tail.3.weight       phase1 |  1.03 (3.4e-03, 3.3e-03) x4 nb1 1x96x128         | 1.3e-06 (1.9e-06) x4 nb1 3x64x96
  tail.3.weight       phase2 |  1.04 (3.8e-03, 3.6e-03) x4 nb1 2x40x56          | 1.2e-06 (1.7e-06) x4 nb1 3x64x96
  tail.3.weight       phase3 |  1.11 (3.5e-03, 3.2e-03) x4 nb1 1x32x32          | 1.1e-06 (1.5e-06) x4 nb1 3x64x96
  tail.3.bias         all    |  1.03 (2.5e-03, 2.4e-03) x4 nb1 1x32x32          | 4.6e-07 (5.0e-06) x4 nb1 3x64x96
  tail.3.bias         phase0 |  1.03 (3.2e-03, 3.1e-03) x4 nb1 3x64x96          | 5.6e-07 (5.1e-06) x4 nb2 2x40x56
  tail.3.bias         phase1 |  1.03 (2.3e-03, 2.3e-03) x4 nb1 1x32x32          | 4.6e-07 (2.6e-06) x4 nb1 2x40x56
  tail.3.bias         phase2 |  1.04 (2.5e-03, 2.4e-03) x4 nb1 1x32x32          | 4.4e-07 (5.6e-06) x4 nb1 3x64x96
  tail.3.bias         phase3 |  1.05 (3.1e-03, 3.0e-03) x4 nb1 1x32x32          | 7.8e-07 (6.8e-06) x4 nb1 3x64x96
  tail.0.weight       all    |  1.02 (6.9e-04, 6.8e-04) x2 nb1 2x40x56          | 9.7e-07 (1.2e-06) x4 nb2 2x40x56
  tail.0.weight       phase0 |  1.00 (9.9e-04, 9.9e-04) x2 nb1 2x40x56          | 1.1e-06 (1.0e-06) x4 nb2 2x40x56
  tail.0.weight       phase1 |  0.96 (2.4e-03, 2.5e-03) x3 nb1 2x40x56          | 1.1e-06 (2.1e-06) x4 nb2 2x40x56
  tail.0.weight       phase2 |  1.05 (6.0e-04, 5.7e-04) x2 nb1 2x40x56          | 7.5e-07 (1.6e-06) x4 nb1 2x40x56
  tail.0.weight       phase3 |  1.06 (1.4e-03, 1.3e-03) x3 nb1 2x40x56          | 1.2e-06 (2.1e-06) x4 nb2 2x40x56
  tail.0.bias         all    |  1.04 (7.3e-04, 7.0e-04) x2 nb1 2x40x56          | 4.4e-07 (2.0e-06) x4 nb1 1x32x32
  tail.0.bias         phase0 |  1.07 (1.4e-07, 1.3e-07) x4 nb1 3x64x96          | 3.8e-07 (1.7e-06) x4 nb1 1x32x32
  tail.0.bias         phase1 |  1.11 (4.6e-08, 4.2e-08) x4 nb1 1x32x32          | 5.2e-07 (3.1e-06) x4 nb1 1x32x32
  tail.0.bias         phase2 |  1.14 (6.7e-04, 5.9e-04) x2 nb1 2x40x56          | 5.3e-07 (2.5e-06) x4 nb1 1x32x32
  tail.0.bias         phase3 |  1.04 (1.6e-03, 1.6e-03) x3 nb1 2x40x56          | 4.5e-07 (2.0e-06) x4 nb1 1x32x32
  body.0.attn1.wqkv   all    |  0.55 (5.2e-08, 9.5e-08) x4 nb1 1x32x32          | 1.4e-06 (8.5e-07) x4 nb1 2x40x56 l1
  body.0.attn1.wqkv   q      |  0.62 (2.7e-07, 4.3e-07) x4 nb1 2x40x56 plain    | 7.0e-07 (1.1e-06) x4 nb1 2x40x56
  body.0.attn1.wqkv   k      |  0.63 (1.0e-07, 1.6e-07) x4 nb2 2x40x56          | 6.6e-07 (1.4e-06) x4 nb1 2x40x56
  body.0.attn1.wqkv   v      |  0.55 (5.2e-08, 9.5e-08) x4 nb1 1x32x32          | 1.4e-06 (8.5e-07) x4 nb1 2x40x56 l1
  body.0.attn2.wqkv   all    |  0.87 (8.8e-08, 1.0e-07) x4 nb1 1x32x32          | 1.3e-06 (1.1e-06) x4 nb1 2x40x56 l1
  body.0.attn2.wqkv   q      |  0.89 (1.3e-07, 1.4e-07) x4 nb1 1x96x128         | 6.6e-07 (1.2e-06) x4 nb1 1x96x128
  body.0.attn2.wqkv   k      |  0.71 (5.2e-08, 7.4e-08) x4 nb1 1x32x32          | 4.2e-07 (1.1e-06) x2 nb1 2x40x56
  body.0.attn2.wqkv   v      |  0.87 (8.9e-08, 1.0e-07) x4 nb1 1x32x32          | 1.3e-06 (1.2e-06) x4 nb1 2x40x56 l1
  body.0.attn3.wqkv   all    |  0.79 (6.7e-08, 8.5e-08) x4 nb1 3x64x96          | 4.5e-06 (5.2e-06) x4 nb1 2x40x56 l1
  body.0.attn3.wqkv   q      |  0.87 (8.5e-08, 9.7e-08) x4 nb1 3x64x96          | 6.7e-07 (7.2e-07) x4 nb1 1x32x32
  body.0.attn3.wqkv   k      |  0.84 (4.3e-08, 5.1e-08) x4 nb1 1x32x32          | 3.0e-07 (5.9e-07) x2 nb1 2x40x56
  body.0.attn3.wqkv   v      |  0.79 (6.2e-08, 7.9e-08) x4 nb1 2x40x56          | 4.6e-06 (5.2e-06) x4 nb1 2x40x56 l1
  body.0.attn4.wqkv   all    |  0.78 (6.6e-08, 8.5e-08) x4 nb1 2x40x56          | 5.2e-06 (5.9e-06) x4 nb1 2x40x56 l1
  body.0.attn4.wqkv   q      |  0.95 (1.2e-07, 1.3e-07) x4 nb1 3x64x96          | 5.5e-07 (9.7e-07) x4 nb1 1x96x128
  body.0.attn4.wqkv   k      |  0.81 (1.6e-07, 2.0e-07) x4 nb1 3x64x96          | 2.9e-07 (5.8e-07) x4 nb1 3x64x96
  body.0.attn4.wqkv   v      |  0.79 (6.6e-08, 8.3e-08) x4 nb1 2x40x56          | 5.2e-06 (5.9e-06) x4 nb1 2x40x56 l1
  body.0.ff.weight    all    |  0.51 (2.8e-07, 5.5e-07) x4 nb1 2x40x56          | 8.0e-07 (1.7e-06) x4 nb1 2x40x56
  body.0.ff.weight    centre |  0.52 (3.1e-07, 6.0e-07) x4 nb1 2x40x56          | 9.3e-07 (2.1e-06) x4 nb1 2x40x56
  body.0.ff.weight    edge   |  0.51 (2.9e-07, 5.7e-07) x4 nb1 2x40x56          | 8.2e-07 (1.7e-06) x4 nb1 2x40x56
  body.0.ff.weight    corner |  0.51 (9.6e-08, 1.9e-07) x4 nb1 1x32x32          | 7.6e-07 (1.6e-06) x4 nb1 2x40x56
  body.0.ff.bias      all    |  1.09 (7.7e-08, 7.1e-08) x4 nb1 2x40x56 plain    | 8.2e-07 (1.8e-06) x4 nb1 2x40x56
  body.0.attn1.rel_h  all    |  1.18 (1.0e-03, 8.9e-04) x4 nb1 2x40x56 l1       | 1.4e-05 (2.3e-05) x4 nb1 2x40x56
  body.0.attn1.rel_h  ring   |  1.20 (1.2e-03, 9.7e-04) x4 nb1 2x40x56 l1       | 1.5e-05 (1.9e-05) x4 nb1 2x40x56
  body.0.attn1.rel_h  inner  |  1.15 (9.1e-04, 7.9e-04) x4 nb1 2x40x56 l1       | 1.2e-05 (2.5e-05) x4 nb1 1x32x32
  body.0.attn1.rel_w  all    |  1.35 (2.4e-02, 1.8e-02) x3 nb1 2x40x56          | 4.1e-05 (3.5e-05) x4 nb1 1x32x32
  body.0.attn1.rel_w  ring   |  1.38 (2.2e-02, 1.6e-02) x3 nb1 2x40x56          | 7.1e-05 (1.6e-05) x4 nb1 1x32x32
  body.0.attn1.rel_w  inner  |  1.29 (4.2e-02, 3.3e-02) x3 nb1 2x40x56          | 3.4e-05 (3.7e-05) x4 nb1 1x32x32
  body.0.attn2.rel_h  all    |  1.03 (1.5e-03, 1.5e-03) x4 nb1 2x40x56 l1       | 4.7e-06 (1.3e-05) x4 nb1 1x32x32
  body.0.attn2.rel_h  ring   |  1.31 (3.4e-04, 2.6e-04) x4 nb1 2x40x56 l1       | 5.3e-06 (9.9e-06) x4 nb1 1x32x32
  body.0.attn2.rel_h  inner  |  1.02 (2.0e-03, 1.9e-03) x4 nb1 2x40x56 l1       | 6.2e-06 (7.7e-06) x4 nb1 3x64x96
  body.0.attn2.rel_w  all    |  1.06 (1.0e-02, 9.6e-03) x4 nb1 2x40x56          | 6.3e-06 (1.8e-05) x4 nb1 1x32x32
  body.0.attn2.rel_w  ring   |  1.09 (3.4e-03, 3.1e-03) x4 nb2 2x40x56          | 9.4e-06 (1.9e-05) x4 nb1 1x32x32
  body.0.attn2.rel_w  inner  |  1.08 (1.3e-02, 1.2e-02) x4 nb1 2x40x56          | 6.9e-06 (1.1e-05) x2 nb1 2x40x56
  body.0.attn3.rel_h  all    |  1.20 (3.9e-03, 3.2e-03) x4 nb1 2x40x56          | 4.5e-06 (6.5e-06) x4 nb1 1x32x32
  body.0.attn3.rel_h  ring   |  1.49 (2.9e-03, 1.9e-03) x4 nb1 2x40x56          | 6.4e-06 (1.5e-05) x3 nb1 2x40x56
  body.0.attn3.rel_h  inner  |  1.18 (4.0e-03, 3.4e-03) x4 nb1 2x40x56          | 4.5e-06 (6.5e-06) x4 nb1 1x32x32
  body.0.attn3.rel_w  all    |  1.10 (1.5e-03, 1.3e-03) x4 nb1 2x40x56 l1       | 6.8e-06 (6.7e-06) x4 nb1 1x96x128
  body.0.attn3.rel_w  ring   |  1.16 (7.4e-03, 6.4e-03) x2 nb1 2x40x56          | 8.1e-06 (4.2e-06) x4 nb2 2x40x56
  body.0.attn3.rel_w  inner  |  1.12 (1.5e-03, 1.3e-03) x4 nb1 2x40x56 l1       | 7.0e-06 (6.1e-06) x4 nb1 1x96x128
  body.0.attn4.rel_h  all    |  1.01 (2.8e-03, 2.8e-03) x4 nb1 2x40x56 l1       | 4.1e-06 (3.8e-06) x3 nb1 2x40x56
  body.0.attn4.rel_h  ring   |  1.03 (2.8e-03, 2.7e-03) x4 nb1 3x64x96          | 6.2e-06 (1.4e-05) x4 nb1 1x32x32
  body.0.attn4.rel_h  inner  |  1.01 (3.1e-03, 3.0e-03) x4 nb1 2x40x56 l1       | 4.1e-06 (3.6e-06) x3 nb1 2x40x56
  body.0.attn4.rel_w  all    |  1.01 (4.2e-03, 4.1e-03) x4 nb1 1x96x128         | 5.3e-06 (7.8e-06) x3 nb1 2x40x56
  body.0.attn4.rel_w  ring   |  1.00 (8.2e-03, 8.2e-03) x4 nb1 1x32x32          | 6.2e-06 (1.4e-05) x4 nb1 1x32x32
  body.0.attn4.rel_w  inner  |  1.01 (4.1e-03, 4.1e-03) x4 nb1 1x96x128         | 5.8e-06 (7.3e-06) x3 nb1 2x40x56
  head.weight         all    |  1.00 (1.7e-03, 1.7e-03) x4 nb1 1x32x32          | 8.1e-07 (1.3e-06) x4 nb1 2x40x56
  head.weight         centre |  1.00 (2.1e-03, 2.1e-03) x4 nb1 1x32x32          | 8.3e-07 (1.4e-06) x4 nb1 2x40x56
  head.weight         edge   |  1.00 (1.6e-03, 1.6e-03) x4 nb1 1x32x32          | 8.0e-07 (1.3e-06) x4 nb1 2x40x56
  head.weight         corner |  1.00 (1.6e-03, 1.6e-03) x4 nb1 1x32x32          | 8.1e-07 (1.3e-06) x4 nb1 2x40x56
  head.bias           all    |  2.24 (9.5e-09, 4.3e-09) x4 nb1 3x64x96          | 1.5e-06 (2.0e-06) x4 nb1 2x40x56
  body.1.attn1.wqkv   all    |  0.46 (7.2e-08, 1.6e-07) x4 nb2 2x40x56          | 2.4e-07 (5.6e-07) x4 nb2 2x40x56
  body.1.attn1.wqkv   q      |  0.61 (1.3e-07, 2.1e-07) x4 nb2 2x40x56          | 1.1e-06 (1.1e-06) x4 nb2 2x40x56
  body.1.attn1.wqkv   k      |  0.57 (1.1e-07, 1.9e-07) x4 nb2 2x40x56          | 2.7e-07 (5.5e-07) x4 nb2 2x40x56
  body.1.attn1.wqkv   v      |  0.46 (7.2e-08, 1.6e-07) x4 nb2 2x40x56          | 2.3e-07 (5.6e-07) x4 nb2 2x40x56
  body.1.attn2.wqkv   all    |  0.55 (9.2e-08, 1.7e-07) x4 nb2 2x40x56          | 6.0e-07 (1.3e-06) x4 nb2 2x40x56
  body.1.attn2.wqkv   q      |  0.54 (9.7e-08, 1.8e-07) x4 nb2 2x40x56          | 1.8e-06 (4.2e-06) x4 nb2 2x40x56
  body.1.attn2.wqkv   k      |  0.55 (5.0e-08, 9.2e-08) x4 nb2 2x40x56          | 1.7e-07 (4.7e-07) x4 nb2 2x40x56
  body.1.attn2.wqkv   v      |  0.55 (9.3e-08, 1.7e-07) x4 nb2 2x40x56          | 5.5e-07 (1.2e-06) x4 nb2 2x40x56
  body.1.attn3.wqkv   all    |  0.77 (6.0e-08, 7.8e-08) x4 nb2 2x40x56          | 2.2e-06 (4.4e-06) x4 nb2 2x40x56
  body.1.attn3.wqkv   q      |  0.53 (8.1e-08, 1.5e-07) x4 nb2 2x40x56          | 1.2e-06 (2.7e-06) x4 nb2 2x40x56
  body.1.attn3.wqkv   k      |  0.58 (5.9e-08, 1.0e-07) x4 nb2 2x40x56          | 3.3e-07 (6.0e-07) x4 nb2 2x40x56
  body.1.attn3.wqkv   v      |  0.77 (6.0e-08, 7.8e-08) x4 nb2 2x40x56          | 2.3e-06 (4.4e-06) x4 nb2 2x40x56
  body.1.attn4.wqkv   all    |  0.75 (5.4e-08, 7.2e-08) x4 nb2 2x40x56          | 1.6e-06 (2.8e-06) x4 nb2 2x40x56
  body.1.attn4.wqkv   q      |  0.81 (7.5e-08, 9.2e-08) x4 nb2 2x40x56          | 1.4e-06 (2.3e-06) x4 nb2 2x40x56
  body.1.attn4.wqkv   k      |  0.69 (6.7e-08, 9.7e-08) x4 nb2 2x40x56          | 3.3e-07 (6.4e-07) x4 nb2 2x40x56
  body.1.attn4.wqkv   v      |  0.75 (5.4e-08, 7.1e-08) x4 nb2 2x40x56          | 1.6e-06 (2.8e-06) x4 nb2 2x40x56
  body.1.ff.weight    all    |  0.44 (2.2e-07, 4.9e-07) x4 nb2 2x40x56          | 1.3e-06 (2.3e-06) x4 nb2 2x40x56
  body.1.ff.weight    centre |  0.44 (2.2e-07, 5.0e-07) x4 nb2 2x40x56          | 8.4e-07 (1.9e-06) x4 nb2 2x40x56
  body.1.ff.weight    edge   |  0.44 (2.2e-07, 5.0e-07) x4 nb2 2x40x56          | 1.3e-06 (2.3e-06) x4 nb2 2x40x56
  body.1.ff.weight    corner |  0.45 (2.2e-07, 4.8e-07) x4 nb2 2x40x56          | 1.4e-06 (2.5e-06) x4 nb2 2x40x56
  body.1.ff.bias      all    |  0.90 (4.2e-08, 4.6e-08) x4 nb2 2x40x56          | 2.1e-07 (5.6e-07) x4 nb2 2x40x56
  body.1.attn1.rel_h  all    |  1.06 (8.3e-03, 7.8e-03) x4 nb2 2x40x56          | 2.5e-06 (3.8e-06) x4 nb2 2x40x56
  body.1.attn1.rel_h  ring   |  1.09 (6.9e-03, 6.3e-03) x4 nb2 2x40x56          | 2.3e-06 (2.3e-06) x4 nb2 2x40x56
  body.1.attn1.rel_h  inner  |  1.05 (8.9e-03, 8.5e-03) x4 nb2 2x40x56          | 2.6e-06 (4.4e-06) x4 nb2 2x40x56
  body.1.attn1.rel_w  all    |  0.84 (6.6e-03, 7.9e-03) x4 nb2 2x40x56          | 2.8e-06 (2.9e-06) x4 nb2 2x40x56
  body.1.attn1.rel_w  ring   |  0.81 (9.3e-03, 1.1e-02) x4 nb2 2x40x56          | 3.5e-06 (3.8e-06) x4 nb2 2x40x56
  body.1.attn1.rel_w  inner  |  0.86 (5.6e-03, 6.5e-03) x4 nb2 2x40x56          | 2.5e-06 (2.6e-06) x4 nb2 2x40x56
  body.1.attn2.rel_h  all    |  1.05 (5.2e-03, 5.0e-03) x4 nb2 2x40x56          | 3.1e-06 (8.1e-06) x4 nb2 2x40x56
  body.1.attn2.rel_h  ring   |  1.01 (4.7e-03, 4.7e-03) x4 nb2 2x40x56          | 2.8e-06 (2.2e-06) x4 nb2 2x40x56
  body.1.attn2.rel_h  inner  |  1.07 (5.5e-03, 5.2e-03) x4 nb2 2x40x56          | 3.4e-06 (1.1e-05) x4 nb2 2x40x56
  body.1.attn2.rel_w  all    |  1.12 (4.4e-03, 3.9e-03) x4 nb2 2x40x56          | 3.1e-06 (7.9e-06) x4 nb2 2x40x56
  body.1.attn2.rel_w  ring   |  0.96 (1.6e-03, 1.7e-03) x4 nb2 2x40x56          | 2.2e-06 (6.3e-06) x4 nb2 2x40x56
  body.1.attn2.rel_w  inner  |  1.12 (5.1e-03, 4.6e-03) x4 nb2 2x40x56          | 3.4e-06 (8.5e-06) x4 nb2 2x40x56
  body.1.attn3.rel_h  all    |  1.01 (1.3e-02, 1.3e-02) x4 nb2 2x40x56          | 7.6e-06 (1.6e-05) x4 nb2 2x40x56
  body.1.attn3.rel_h  ring   |  0.95 (8.2e-03, 8.6e-03) x4 nb2 2x40x56          | 2.6e-06 (1.1e-05) x4 nb2 2x40x56
  body.1.attn3.rel_h  inner  |  1.01 (1.4e-02, 1.4e-02) x4 nb2 2x40x56          | 8.6e-06 (1.7e-05) x4 nb2 2x40x56
  body.1.attn3.rel_w  all    |  0.99 (1.5e-02, 1.5e-02) x4 nb2 2x40x56          | 1.2e-05 (1.8e-05) x4 nb2 2x40x56
  body.1.attn3.rel_w  ring   |  0.93 (6.1e-03, 6.5e-03) x4 nb2 2x40x56          | 5.0e-06 (1.9e-05) x4 nb2 2x40x56
  body.1.attn3.rel_w  inner  |  1.00 (1.8e-02, 1.8e-02) x4 nb2 2x40x56          | 1.4e-05 (1.7e-05) x4 nb2 2x40x56
  body.1.attn4.rel_h  all    |  1.00 (5.3e-03, 5.3e-03) x4 nb2 2x40x56          | 4.5e-06 (6.2e-06) x4 nb2 2x40x56
  body.1.attn4.rel_h  ring   |  1.00 (4.3e-03, 4.3e-03) x4 nb2 2x40x56          | 5.6e-06 (8.7e-06) x4 nb2 2x40x56
  body.1.attn4.rel_h  inner  |  1.00 (5.4e-03, 5.4e-03) x4 nb2 2x40x56          | 4.4e-06 (5.9e-06) x4 nb2 2x40x56
  body.1.attn4.rel_w  all    |  1.00 (7.3e-03, 7.3e-03) x4 nb2 2x40x56          | 8.1e-06 (1.6e-05) x4 nb2 2x40x56
  body.1.attn4.rel_w  ring   |  1.01 (4.4e-03, 4.4e-03) x4 nb2 2x40x56          | 2.4e-06 (1.6e-05) x4 nb2 2x40x56
  body.1.attn4.rel_w  inner  |  1.00 (7.9e-03, 7.9e-03) x4 nb2 2x40x56          | 9.0e-06 (1.6e-05) x4 nb2 2x40x56
  tail.3.weight       centre |  1.00 (1.5e-04, 1.5e-04) x2 nb1 2x40x56          | 3.0e-07 (1.1e-06) x3 nb1 2x40x56
  tail.3.weight       edge   |  1.03 (3.0e-04, 2.9e-04) x2 nb1 2x40x56          | 3.8e-07 (1.2e-06) x3 nb1 2x40x56
  tail.3.weight       corner |  1.01 (7.0e-04, 6.9e-04) x3 nb1 2x40x56          | 3.5e-07 (9.1e-07) x2 nb1 2x40x56
  tail.0.weight       phase4 |  1.06 (1.9e-03, 1.8e-03) x3 nb1 2x40x56          | 3.4e-07 (7.0e-07) x3 nb1 2x40x56
  tail.0.weight       phase5 |  1.00 (2.1e-03, 2.1e-03) x3 nb1 2x40x56          | 3.5e-07 (6.5e-07) x3 nb1 2x40x56
  tail.0.weight       phase6 |  1.00 (1.9e-03, 1.9e-03) x3 nb1 2x40x56          | 3.5e-07 (5.9e-07) x3 nb1 2x40x56
  tail.0.weight       phase7 |  1.05 (1.7e-03, 1.7e-03) x3 nb1 2x40x56          | 3.5e-07 (6.6e-07) x3 nb1 2x40x56
  tail.0.weight       phase8 |  1.00 (2.6e-03, 2.6e-03) x3 nb1 2x40x56          | 4.1e-07 (6.4e-07) x3 nb1 2x40x56
  tail.0.bias         phase4 |  0.97 (2.0e-03, 2.1e-03) x3 nb1 2x40x56          | 2.2e-07 (1.1e-06) x3 nb1 2x40x56
  tail.0.bias         phase5 |  0.96 (2.0e-03, 2.1e-03) x3 nb1 2x40x56          | 1.8e-07 (1.3e-06) x3 nb1 2x40x56
  tail.0.bias         phase6 |  1.00 (1.7e-03, 1.7e-03) x3 nb1 2x40x56          | 2.1e-07 (1.5e-06) x3 nb1 2x40x56
  tail.0.bias         phase7 |  1.00 (1.7e-03, 1.7e-03) x3 nb1 2x40x56          | 2.0e-07 (1.9e-06) x3 nb1 2x40x56
  tail.0.bias         phase8 |  1.00 (3.1e-03, 3.1e-03) x3 nb1 2x40x56          | 2.5e-07 (1.0e-06) x3 nb1 2x40x56
"""
import pytest
import torch

from oracle import m2trans_oracle as O
from tests import bwd_stage_ref as R
from tests.gpu_util import build_model, hip_backward_trace, hip_forward_trace

pytestmark = pytest.mark.gpu


def _set(plan, key, value):
    from m2trans_amd import _lib
    _lib.check(_lib.load().m2t_set_option(plan.handle, key.encode(), int(value)), "m2t_set_option " + key)


def _step(model, x, w, hr):
    """One forward + backward through autograd (tests/test_gpu_input_grad.py _step); returns (lr.grad, sr, g(sr), {parameter: grad})."""
    model.zero_grad(set_to_none=True)
    lr = x.detach().clone().requires_grad_(True)
    sr = model(lr)
    seen = {}
    sr.register_hook(lambda g: seen.__setitem__("g_sr", g.detach().clone()))
    loss = (sr * w).sum() if w is not None else torch.nn.L1Loss()(sr, hr)
    loss.backward()
    torch.cuda.synchronize()
    pg = {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.requires_grad}
    return lr.grad.detach().clone(), sr.detach(), seen["g_sr"], pg


def _is_param(name):
    return name.startswith(("head.", "body.", "tail."))


def _gate(scale, nb, B, H0, W0, dtype, loss_kind="smooth", opts=None, entries=None):
    """opts: plan options set before the first step; entries: predicate on the entry name -- the gated (and required) entries, default all."""
    model, p = build_model(scale, nb, dtype)
    x = O.closed_form_image(B, 3, H0, W0)
    xd = x.cuda()
    w = hr = None
    if loss_kind == "smooth":
        w = R.cotangent(B, H0 * scale, W0 * scale).float().cuda()
    else:       # part of the output under the clamp (tests/test_gpu_input_grad.py)
        hr = (O.closed_form_image(B, 3, H0 * scale, W0 * scale, phase=0.7) * 1.2 - 0.1).clamp(0, 1).cuda()
    plan = model._plan_for(xd)
    for k, v in (opts or {}).items():
        _set(plan, k, v)
    H, W = plan.query("padded_h"), plan.query("padded_w")
    extra = {}
    if dtype == "bf16":
        # the default tails keep gelu / gelu' of their last expansion in LDS or registers; the stored-form run gives the same forward
        # bits (tests/test_gpu_baseline_configs.py check_vs_oracle) and its workspace feeds the teacher-forced oracle
        names, stored = (("t2act", "t2der"), 1) if scale == 4 else (("t1act", "t1der"), 0)
        if plan.query("stores_t2" if scale == 4 else "stores_t1") == 0:
            default = plan.query("opt:fused_tail")
            _set(plan, "fused_tail", stored)
            _, sr_stored, _, _ = _step(model, xd, w, hr)
            tr = hip_forward_trace(plan, scale, nb, B, H, W)
            extra = {n: tr[n] for n in names}
            _set(plan, "fused_tail", default)
            assert plan.query("stores_t2" if scale == 4 else "stores_t1") == 0
    # the first backward after an option change publishes the reduction table and reduces everything at its end on the side stream
    gx, sr, g_sr, pg = _step(model, xd, w, hr)
    if extra:
        assert torch.equal(sr, sr_stored), "the stored-form tail is not bit-identical in the forward pass"
    if loss_kind == "l1":
        assert bool(((sr <= 0) | (sr >= 1)).any())           # the clamp is live in this case
    ftrace = dict(hip_forward_trace(plan, scale, nb, B, H, W), **extra)
    taps = hip_backward_trace(plan, scale, nb, B, H, W)
    taps["lr.grad"] = gx.cpu()
    assert set(pg) == set(O.trainable_names(p))
    taps.update({n: v.cpu() for n, v in pg.items()})
    # steady state: the second backward reduces as it goes through the published table and runs the head's weight gradient and its
    # reduction on the main stream; nothing accumulates with atomics, so every parameter gradient is bit-equal to the first pass
    gx2, _, _, pg2 = _step(model, xd, w, hr)
    diff = [n for n in pg if not torch.equal(pg[n], pg2[n])]
    assert not diff and torch.equal(gx, gx2), f"second backward differs from the first in {diff}"
    if opts and "wgrad_big_tiles" in opts:
        assert plan.query("opt:wgrad_big_tiles") == 1000 + opts["wgrad_big_tiles"]
    del model
    force = ftrace if dtype == "bf16" else None
    g64 = R.build_graph(x, p, scale, nb, dtype, force=force, leaf_params=True)
    g32 = R.build_graph(x, p, scale, nb, dtype, force=force, ftype=torch.float32, leaf_params=True)
    gpre_ref = R.seed(g_sr.cpu().double(), ftrace["srpre"].double())
    err, refs = R.stage_errors(g64, taps, gpre_ref)
    o32 = R.oracle32_errors(g64, g32, taps, refs, gpre_ref)
    required = {"gT", "gn[1]", "gn[2]", "gn[3]", "gn[4]", "b0.gqkv1", "b0.gqkv2", "b0.gqkv3", "b0.gqkv4", "gres", "lr.grad", "gpre"}
    required |= ({"g_t1pre"} if scale == 4 else set()) | ({"gB", "b1.gqkv1", "b1.gqkv2", "b1.gqkv3", "b1.gqkv4"} if nb == 2 else set())
    required |= set(O.trainable_names(p))
    if entries is not None:
        required = {n for n in required if entries(n)}
        err = {k: e for k, e in err.items() if entries(k[0])}
    assert required <= {k[0] for k in err}, required - {k[0] for k in err}
    if dtype == "bf16":
        bad, table = R.gate_bf16(err, R.budget(g64, taps["gpre"], taps), floor=o32)
    else:
        bad, table = R.gate_fp32(err, o32)
    print(f"\nx{scale} nb={nb} {B}x{H0}x{W0} {dtype} {loss_kind}{' ' + str(opts) if opts else ''}: error, " +
          ("budget, error / budget" if dtype == "bf16" else "float32 oracle's error, ratio"))
    print(R.format_table(table))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,H0,W0", [(1, 32, 32), (2, 40, 56), (3, 64, 96), (1, 96, 128)])
def test_x4_one_block(B, H0, W0, dtype):
    """1x32x32: a single level-2 window, every ring key a phantom; 2x40x56: reflect-padded to 64x64, 2x2 level-2 windows, pad fold live;
    3x64x96: odd B, 2x3; 1x96x128: 3x4, the first shape with an interior level-2 window."""
    _gate(4, 1, B, H0, W0, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_x4_one_block_l1_with_the_clamp_live(dtype):
    _gate(4, 1, 2, 40, 56, dtype, loss_kind="l1")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_x4_two_blocks(dtype):
    """The non-last block, the gB tap and buffer set 1."""
    _gate(4, 2, 2, 40, 56, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("scale", [2, 3])
def test_x2_x3_one_block(scale, dtype):
    """The streaming tails' gpre -> gT."""
    _gate(scale, 1, 2, 40, 56, dtype)


def test_x4_one_block_big_wgrad_tiles():
    """wgrad_tn_big_kernel (128 x 128 output tiles; by itself only from 24 576 rows) forced at 2x40x56: level-2 M = 512 rows, N x K =
    768 x 256, four slabs of one 128-row stage -- the C = 256 qkv weight gradients of that kernel against fp64."""
    _gate(4, 1, 2, 40, 56, "bf16", opts={"wgrad_big_tiles": 256})


def test_x4_one_block_plain_bf16_kernels():
    """attn_bwd = 0, fused_conv_bwd = 0, fused_tail = 0 (PLAIN_BF16 of tests/test_gpu_schedule.py): conv3x3_c64_wgrad, final_conv_wgrad and the
    UNSHUF wgrad_tn of tail.3 in their bf16 instantiation.  Taps under these options (backward_impl, csrc/m2t_api.hip): TAIL_BWD_PLAIN
    stores g_t2pre (final_conv_dgrad), g_t1pre and gT (the two gemm_nt) in regions of their own; conv3x3_c64 writes gxc; each branch's
    window_attn_bwd completes dK | dV in its own gqkv buffer with its own halo gather on the main stream, gemm_nt writes gd (shared, not a
    tap) and branch_prep_bwd the branch's plane of gn; launch_instnorm_bwd of block 0 then writes g(res) over gxc.  So gpre, g_t1pre,
    gT, b0.gqkv<i>, gn and gres are intact, as in the default schedule, and every parameter has its cotangent.  What is NOT carried over
    is the budget of whatever passes through the generic window_attn_bwd_kernel<bf16_t>: it holds P AND dP in bf16 in LDS, rounding
    points that tests/attn_ref.py states for the resident kernels only -- the data taps and the rel-pos tables are therefore left to the
    default cells, and this cell gates the weight and bias gradients, whose stages are the same arithmetic on either schedule: one
    float32-accumulating kernel on the stored taps, or geff / gt2 for tail.3."""
    _gate(4, 1, 2, 40, 56, "bf16", opts={"attn_bwd": 0, "fused_conv_bwd": 0, "fused_tail": 0},
          entries=lambda n: _is_param(n) and ".rel_" not in n)
