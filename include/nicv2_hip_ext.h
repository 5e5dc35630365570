/* Entries added after the 86 of nicv2_hip.h live here: that header's function set is closed (its tests count it), this one grows.  Same
 * library (libnicv2_hip.so), same ABI version (additive entries do not bump it), same types, error codes and conventions: include this
 * header instead of nicv2_hip.h to get both. */
#ifndef NICV2_HIP_EXT_H
#define NICV2_HIP_EXT_H

#include "nicv2_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- B hash-grid fields per launch with the decoder on the 16-bit matrix pipe (hashgrid.py, hash_batch_forward_p16, HashGridFieldBatch.decode /
 *      query / resample(precision=); csrc/hashgrid_fused16.hip).  Forward only: one launch, no atomics - the same call gives the
 *      same bits.  nic_hash_batch_forward_p16 is nic_hash_fused_forward_p16 per field in ONE launch, bit for bit (the same gather, the same
 *      products in the same order from zero accumulators), with nic_hash_batch_forward_source's contract: the stacked source (src->data the BASE
 *      of n_fields tables without gaps, field b's b x stride bytes after it, stride as there; a BITS base 4-byte aligned), the stacked decoder
 *      (the bases of W1 [B, 64, L F], b1 [B, 64], W2 [B, 64, 64], b2 [B, 64], W3 [B, 3, 64], b3 [B, 3]), exactly one of origins [B, num_crops,
 *      dim] int32 / points [B, n_points, dim] fp32 (sample units, the clamping of nic_hash_encode_points; then desc->extent is the FIELD size and
 *      desc->num_crops is 1), y = [B, N, 3] or [B, n_points, 3] in that entry's order.  precision = NIC_HASH_PREC_SPLIT or NIC_HASH_PREC_BF16 as
 *      in nic_hash_fused_forward_p16.
 *      groups_per_field = G on the wave items of ONE field (its patches, or ceil(n_points / 64)) with the rule of nic_hash_batch_forward_source
 *      on the 16-bit kernel's workgroup cap: one workgroup per CU at levels x features > 32, two at <= 32 (its LDS is 61 KB there).  0 is
 *      automatic: cap / n_fields rounded up to a multiple of 8, at least 8, at most the grid nic_hash_fused_forward_p16 would use for one
 *      field's items; a positive G must be a multiple of 8 and at most that grid.
 *      Host checks, all before any GPU work, in nic_hash_batch_forward_source's order with the precision after the source: null desc / mlp
 *      (NIC_E_NULL); the fused set (nic_hash_fused_supported's code); both or neither of origins / points (NIC_E_ARG); the descriptor of that
 *      position source (points: num_crops == 1, NIC_E_SHAPE, and 256 S_max < 2^30, NIC_E_ARG; origins: 256 S_max < 2^30, NIC_E_ARG); n_fields
 *      in 1 .. 65535 (NIC_E_ARG); groups_per_field (NIC_E_ARG; for this check alone n_points <= 0 counts as one wave item); null src,
 *      src->data, decoder layer or y (NIC_E_NULL); the source (NIC_E_ARG: kind, num_bits, alignment, in nic_hash_encode_points' order);
 *      precision (NIC_E_ARG); n_points < 0 with points (NIC_E_ARG); n_points == 0 with points is NIC_OK without a launch. */
int nic_hash_batch_forward_p16(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_hash_source *src,
                               const int32_t *origins, const float *points, int64_t n_points, const nic_mlp *mlp, int precision, float *y,
                               void *stream);

/* ---- B hash-grid fields per launch TRAINED at their own points (hashgrid.py, hash_batch_forward_backward_points, HashGridFieldBatch.train_points /
 *      fit_points; csrc/hashgrid_batch.hip, hash_batch_points_kernel).  nic_hash_batch_forward_backward_points is
 *      nic_hash_fused_forward_backward_points per field in TWO launches whatever n_fields is (the training kernel and the fixed-order reduction
 *      of its records): the contract of nic_hash_batch_forward_backward - stacked tables / table_grads [B, L, T, F], the stacked decoder and its
 *      gradients, loss [B], table_grads ADDED to with fp32 atomics (null: frozen tables, no scatter), the decoder gradients and loss overwritten
 *      or added to under flags = NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS, no optimiser tail, nic_mark_kernel_end honoured - with the
 *      position source of nic_hash_batch_forward_source(points=): desc->extent is the FIELD size and desc->num_crops is 1; points =
 *      [B, n_points, dim] fp32 on the device in sample units with the clamping of nic_hash_encode_points; target and y (y may be null) =
 *      [B, n_points, 3].
 *      Point sets are ragged: counts is null (every field has n_points points) or int32 [B] on the device, field b's own count n_b, clamped to
 *      [0, n_points].  Field b reads the first n_b rows of its points and targets only; rows of y at or past n_b are NOT written; loss[b] =
 *      loss_scale mean((y_b - target_b)^2) over ITS n_b points.  A field with n_b = 0 has loss 0 and decoder gradients written as 0 (both
 *      unchanged under the ADD flags); its table gradient is untouched.
 *      order is null or int32 [B, n_points] of field-LOCAL row indices: wave w of field b takes the rows order[b, 64 w ..].  Only the first n_b
 *      of a row of order are read, each clamped to [0, n_b - 1].  Targets, outputs and the noise of `quant` stay keyed by the row (sample_base
 *      + the row inside the field, and the column): field b sees the noise of a single-field call with the same quant, whatever the order.
 *      groups_per_field = G on the wave items of one field's padded row, ceil(n_points / 64), with nic_hash_batch_forward_source's rule.
 *      workspace >= nic_hash_batch_points_workspace_bytes (n_fields x G records; 0: one of the checks below refuses).
 *      Host checks, all before any GPU work, in nic_hash_batch_forward_backward's order, then the points': null desc / mlp (NIC_E_NULL); the
 *      fused set (nic_hash_fused_supported's code; then 256 S_max < 2^30, NIC_E_ARG); n_fields in 1 .. 65535 (NIC_E_ARG); groups_per_field
 *      (NIC_E_ARG; for this check alone n_points <= 0 counts as one wave item); null tables, points, decoder layer, target, mlp_grads, loss or
 *      workspace (NIC_E_NULL; counts, order, table_grads and y may be null); flags (NIC_E_ARG); quant (nic_hash_fused_forward_backward's
 *      rules); the workspace (NIC_E_WORKSPACE); the descriptor of a point source (num_crops == 1, NIC_E_SHAPE); n_points < 0 or >= 2^31
 *      (NIC_E_ARG); n_points == 0 is NIC_OK without a launch, nothing written. */
size_t nic_hash_batch_points_workspace_bytes(const nic_hash_desc *desc, int n_fields, int groups_per_field, int64_t n_points,
                                             const nic_mlp *mlp);   /* 0: refused */
int nic_hash_batch_forward_backward_points(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_hash_quant *quant,
                                           const float *tables, const float *points, int64_t n_points, const int32_t *counts,
                                           const int32_t *order, const nic_mlp *mlp, const float *target, float loss_scale, float *table_grads,
                                           const nic_mlp_grads *mlp_grads, float *loss, float *y, int flags, void *workspace,
                                           size_t workspace_bytes, void *stream);

/* ---- B hash-grid fields per launch with a level of detail PER POINT, decoded and trained (hashgrid.py, hash_batch_forward_points_lod,
 *      hash_batch_forward_backward_points_lod, HashGridFieldBatch.query / resample / train_points / fit_points(lod=), decode_mip, fit_mips;
 *      csrc/hashgrid_batch.hip, hash_batch_decode_lod_kernel and hash_batch_points_lod_kernel).  The nic_hash_lod section of
 *      nicv2_hip.h holds for every field of the launch, word for word: lambda of point n of field b = (lod ? lod[b, n] : 0) + lod_uniform in
 *      fp32, NaN becomes 0, the sum clamped to [0, 32]; a_l = min(max((fade[l] - lambda) + 1.0f, 0), 1); column l F + f of the row is
 *      fl(a_l r); a level of weight 0 is not read, gets no noise and no atomic, and a level no lane of a wave weighs above 0 costs that wave
 *      no gather; the backward is straight-through, fl(a_l dx) goes where the entry without _lod sends dx.  One nic_hash_lod (fade and
 *      lod_uniform) serves all fields.  lod is NULL or fp32 [B, n_points] on the device (the host never reads it), field b's slice its
 *      n_points values; it is read at the field-local ROW, as the point is: with an `order`, at order[b, pos] clamped to [0, n_b - 1].
 *      Everything else is the sibling's, argument for argument:
 *      nic_hash_batch_forward_points_lod = nic_hash_batch_forward_source with points (no origins: a level of detail is served at points only) -
 *      the stacked source of any of the three kinds, the stacked decoder, points [B, n_points, dim], y [B, n_points, 3], groups_per_field on
 *      ceil(n_points / 64) wave items; one launch, no atomics, the same call gives the same bits; y of field b is
 *      nic_hash_fused_forward_points_lod's on field b's tensors bit for bit.
 *      nic_hash_batch_forward_backward_points_lod = nic_hash_batch_forward_backward_points - counts, order, records, the fixed-order
 *      reduction, flags, noise keys (sample_base + the row inside the field), loss[b] over ITS n_b points, rows of y at or past n_b not
 *      written, nic_mark_kernel_end honoured; the workspace query is nic_hash_batch_points_workspace_bytes.
 *      Host checks, all before any GPU work, in the sibling's order and with its codes; on top of them lodp == NULL is NIC_E_NULL (with the
 *      other pointers), and right after the pointers a fade[l] (l < levels) that is not finite or is negative, a lod_uniform that is not
 *      finite, or reserved != 0 is NIC_E_ARG.  In full, forward: null desc / mlp (NIC_E_NULL); the fused set (nic_hash_fused_supported's
 *      code); the descriptor of a point source (num_crops == 1, NIC_E_SHAPE, and 256 S_max < 2^30, NIC_E_ARG); n_fields in 1 .. 65535
 *      (NIC_E_ARG); groups_per_field (NIC_E_ARG; n_points <= 0 counts as one wave item); null lodp, src, src->data, points, decoder layer or
 *      y (NIC_E_NULL); the nic_hash_lod (NIC_E_ARG); the source (NIC_E_ARG: kind, num_bits, alignment); n_points < 0 (NIC_E_ARG); n_points ==
 *      0 is NIC_OK without a launch.  Training: null desc / mlp; the fused set, then 256 S_max < 2^30; n_fields; groups_per_field; null
 *      lodp, tables, points, decoder layer, target, mlp_grads, loss or workspace (lod, counts, order, table_grads and y may be null); the
 *      nic_hash_lod; flags; quant; the workspace (NIC_E_WORKSPACE); num_crops == 1 (NIC_E_SHAPE); n_points < 0 or >= 2^31 (NIC_E_ARG);
 *      n_points == 0 is NIC_OK without a launch, nothing written. */
int nic_hash_batch_forward_points_lod(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_hash_lod *lodp,
                                      const nic_hash_source *src, const float *points, const float *lod, int64_t n_points, const nic_mlp *mlp,
                                      float *y, void *stream);
int nic_hash_batch_forward_backward_points_lod(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_hash_lod *lodp,
                                               const nic_hash_quant *quant, const float *tables, const float *points, const float *lod,
                                               int64_t n_points, const int32_t *counts, const int32_t *order, const nic_mlp *mlp,
                                               const float *target, float loss_scale, float *table_grads, const nic_mlp_grads *mlp_grads,
                                               float *loss, float *y, int flags, void *workspace, size_t workspace_bytes, void *stream);

/* ---- B hash-grid fields per launch with the gradient with respect to the POINT COORDINATES, alone and in the training step (hashgrid.py,
 *      hash_batch_points_grad, hash_batch_forward_backward_points_grad, HashGridFieldBatch.point_gradient / jacobian / query_differentiable /
 *      train_points_grad / train_points_differentiable; csrc/hashgrid_batch_grad.hip, hash_batch_points_grad_kernel; csrc/hashgrid_batch.hip,
 *      hash_batch_points_joint_kernel).  Both take a NULLABLE nic_hash_lod, as nic_hash_fused_forward_backward_points_grad
 *      does: lodp == NULL is the plain call (and lod != NULL is then NIC_E_ARG), else the nic_hash_lod section of nicv2_hip.h holds for every
 *      field as in the _lod entries above, lod NULL or fp32 [B, n_points] read at the field-local ROW.  dpoints = [B, n_points, dim] fp32: the
 *      derivative of the multilinear interpolant at the rounded position the forward uses, in sample units; an axis whose floating-point
 *      clamp moved the point (or a NaN) gets exactly 0.0f; noise and level weights are constants.  counts and order as in
 *      nic_hash_batch_forward_backward_points: counts null or int32 [B] clamped to [0, n_points], order null or int32 [B, n_points] of
 *      field-local rows, the first n_b read, each clamped to [0, n_b - 1].  Row order[b, pos] of y and dpoints is written once, by the lane
 *      that handles it - overwritten, never added to; rows at or past n_b, and rows an order does not name, are NOT written; a field with
 *      n_b = 0 walks nothing and writes nothing.
 *      nic_hash_batch_points_grad = nic_hash_fused_points_grad per field in ONE launch: no atomics, no workspace, no reduction (tables and
 *      decoders are constants), the same call gives the same bits, and with dy field b's rows are nic_hash_fused_points_grad's on field b's
 *      tensors bit for bit.  The stacked source of any of the three kinds under nic_hash_batch_forward_source's contract and alignment rules,
 *      the stacked decoder, points [B, n_points, dim], exactly one of dy / target [B, n_points, 3], y [B, n_points, 3] or null.  With target,
 *      field b's output gradient is 2 (y - target) loss_scale / (3 n_b), n_b its OWN count.  groups_per_field on ceil(n_points / 64) wave
 *      items, nic_hash_batch_forward_source's rule.
 *      Host checks, all before any GPU work: null desc / mlp (NIC_E_NULL); the fused set (nic_hash_fused_supported's code); the descriptor
 *      of a point source (num_crops == 1, NIC_E_SHAPE, and 256 S_max < 2^30, NIC_E_ARG); n_fields in 1 .. 65535 (NIC_E_ARG);
 *      groups_per_field (NIC_E_ARG; n_points <= 0 counts as one wave item); null src, src->data, points, decoder layer or dpoints
 *      (NIC_E_NULL; lodp, lod, counts, order, dy, target and y may be null); the source (NIC_E_ARG: kind, num_bits, alignment); lod without
 *      lodp, then the nic_hash_lod (NIC_E_ARG); both or neither of dy / target (NIC_E_ARG); n_points < 0 or >= 2^31 (NIC_E_ARG); n_points
 *      == 0 is NIC_OK without a launch, nothing written.
 *      nic_hash_batch_forward_backward_points_grad = nic_hash_batch_forward_backward_points with lodp == NULL, otherwise
 *      nic_hash_batch_forward_backward_points_lod, argument for argument, in the same TWO launches: their records and fixed-order reduction
 *      without a tail, their flags and workspace (nic_hash_batch_points_workspace_bytes), noise keyed by sample_base + the row,
 *      nic_mark_kernel_end honoured, table_grads == NULL frozen tables (no scatter; dpoints and the decoder records are still produced).
 *      On top of their outputs it writes dpoints, the derivative of the loss the call returns for field b taken at the parameters the
 *      forward used - nic_hash_batch_points_grad's with target on the same tables when there is no noise, bit for bit -, overwritten
 *      whatever NIC_HASH_FUSED_ADD_GRADS says.
 *      Host checks, all before any GPU work, in the siblings' order: null desc / mlp (NIC_E_NULL); the fused set, then 256 S_max < 2^30
 *      (NIC_E_ARG); n_fields in 1 .. 65535 (NIC_E_ARG); groups_per_field (NIC_E_ARG; n_points <= 0 counts as one wave item); null tables,
 *      points, decoder layer, target, mlp_grads, loss, dpoints or workspace (NIC_E_NULL; lodp, lod, counts, order, table_grads and y may be
 *      null); lod without lodp, then the nic_hash_lod (NIC_E_ARG); flags (NIC_E_ARG); quant (nic_hash_fused_forward_backward's rules); the
 *      workspace (NIC_E_WORKSPACE); num_crops == 1 (NIC_E_SHAPE); n_points < 0 or >= 2^31 (NIC_E_ARG); n_points == 0 is NIC_OK without a
 *      launch, nothing written. */
int nic_hash_batch_points_grad(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_hash_lod *lodp,
                               const nic_hash_source *src, const float *points, const float *lod, int64_t n_points,
                               const int32_t *counts, const int32_t *order, const nic_mlp *mlp, const float *dy,
                               const float *target, float loss_scale, float *y, float *dpoints, void *stream);
int nic_hash_batch_forward_backward_points_grad(const nic_hash_desc *desc, int n_fields, int groups_per_field,
                                                const nic_hash_lod *lodp, const nic_hash_quant *quant, const float *tables,
                                                const float *points, const float *lod, int64_t n_points, const int32_t *counts,
                                                const int32_t *order, const nic_mlp *mlp, const float *target, float loss_scale,
                                                float *table_grads, const nic_mlp_grads *mlp_grads, float *loss, float *y, float *dpoints,
                                                int flags, void *workspace, size_t workspace_bytes, void *stream);

/* ---- The gradient with respect to the LEVEL OF DETAIL of a point, next to the one with respect to its coordinates (hashgrid.py,
 *      hash_encode_points_grad_lod, hash_fused_points_grad_lod, HashGridField.point_gradient_lod / jacobian_lod / query_differentiable_lod;
 *      csrc/hashgrid_lodgrad.hip).  nic_hash_encode_points_grad_lod is nic_hash_encode_points_grad and
 *      nic_hash_fused_points_grad_lod is nic_hash_fused_points_grad, argument for argument, with dlod after dpoints: the same gathers, y and
 *      dpoints of the siblings called with the same nic_hash_lod bit for bit, one launch, no atomics - the same call gives the same bits.
 *      Notation of nic_hash_encode_points_lod: lambda_raw = (lod ? lod[n] : 0) + lod_uniform in fp32; lambda is lambda_raw with NaN -> 0,
 *      clamped to [0, 32]; a_raw = (fade[l] - lambda) + 1.0f in fp32, in exactly that order (the level weight before its clamp).  Level l is
 *      ON THE RAMP iff 0 < a_raw <= 1 - the right-hand derivative, "what happens when the footprint grows": a level exactly at its fade start
 *      (a_raw == 1) has slope -1, a level exactly at its end (a_raw == 0) has slope 0 and is not gathered.  An integer lambda with the
 *      default fades hits these kinks exactly; the convention is part of the contract.
 *          dlod[n] = - sum_{l on the ramp} sum_f g[n, l F + f] r[n, l, f]
 *      g = d loss / d row, the gradient of the WEIGHED column (dx of the layer-wise entry; the decoder's backward of the fused one);
 *      r = the unweighed blend sum_c prod_a cw_a(c) value[l, idx(v + c), f] from the fp32, uint8 or bit-packed table.  Noise does not
 *      enter: these entries have no quant.  dlod[n] is exactly 0.0f when lambda_raw < 0, lambda_raw >= 32 or lambda_raw is NaN (the
 *      right-hand derivative of the clamp); lambda_raw == 0 passes the gradient through.  Positions enter only through r, taken at the
 *      rounded and clamped position the forward uses: a clamped axis does not zero dlod.  dlod = [n_points] fp32 on the device, row n
 *      WRITTEN (never added to) by the lane of point n; nothing past n_points is touched.  The gradient for lod_uniform is the sum of dlod;
 *      the caller forms it.  There is no gradient with respect to fade and no second derivative; the training-step and batched forms are the
 *      sections below.
 *      Host checks, all before any GPU work, are the siblings' in the siblings' order with two changes: lodp == NULL is NIC_E_NULL,
 *      reported with the other pointers (these are _lod entries), and dlod == NULL is NIC_E_NULL.  Layer-wise: the descriptor of a point
 *      source (check of nic_hash_encode_points: NIC_E_NULL / NIC_E_ARG / NIC_E_SHAPE); null lodp, src, src->data, points, dx, dpoints or
 *      dlod (NIC_E_NULL; lod may be null); the source (NIC_E_ARG: kind, num_bits, alignment); the nic_hash_lod (NIC_E_ARG: a fade[l], l <
 *      levels, not finite or negative, lod_uniform not finite, reserved != 0); n_points < 0 (NIC_E_ARG); n_points == 0 is NIC_OK without a
 *      launch.  Fused: null desc / mlp (NIC_E_NULL); the fused set (nic_hash_fused_supported's code); the descriptor of a point source;
 *      null lodp, src, src->data, points, dpoints or dlod, then a null decoder layer (NIC_E_NULL; lod, dy, target and y may be null); the
 *      source; the nic_hash_lod; both or neither of dy / target (NIC_E_ARG); n_points < 0 (NIC_E_ARG); n_points == 0 is NIC_OK without a
 *      launch. */
int nic_hash_encode_points_grad_lod(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_source *src, const float *points,
                                    const float *lod, int64_t n_points, const float *dx, float *dpoints, float *dlod, void *stream);
int nic_hash_fused_points_grad_lod(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_source *src, const float *points,
                                   const float *lod, int64_t n_points, const nic_mlp *mlp, const float *dy, const float *target,
                                   float loss_scale, float *y, float *dpoints, float *dlod, void *stream);

/* ---- The gradient with respect to the LEVEL OF DETAIL from the TRAINING STEP (hashgrid.py, hash_fused_forward_backward_points_grad_lod,
 *      hash_encode_points_grad_lod_noisy, HashGridField.train_points_grad_lod / train_points_differentiable_lod; csrc/hashgrid_lodtrain.hip;
 *      DESIGN 4.7.23).  Notation of the section above: lambda_raw, lambda, a_raw = (fade[l] - lambda) + 1.0f in fp32 in that order; level l is
 *      ON THE RAMP iff 0 < a_raw <= 1; passes(n) iff 0 <= lambda_raw < 32.  The row a training step decodes carries the codec noise INSIDE
 *      the weighed column - column l F + f is a_l (r[n, l, f] + nz[n, l F + f]) - so the slope on the ramp is -(r + nz), not -r:
 *          dlod[n] = passes(n) ? - sum_{l on the ramp} sum_f g[n, l F + f] (r[n, l, f] + nz[n, l F + f]) : 0
 *      g = d loss / d row of the loss the call returns, loss_scale mean((y - target)^2), taken at the parameters the forward used, before
 *      the tail's step (the layer-wise entry: dx); r = the unweighed blend at the rounded, clamped position; nz = exactly the noise value
 *      the forward added to that column: the same key sample_base + n with n the CALLER'S ROW (order[pos] with an order), the same generator
 *      block, the same byte of it; nz is 0 without noise.  The kink rules of the section above hold unchanged: the right-hand derivative,
 *      a_raw == 1 has slope -1, a_raw == 0 has slope 0 and is not gathered, dlod is exactly 0.0f where lambda is clamped or NaN, a clamped
 *      axis zeroes its dpoints and not dlod.  Row n of dpoints and dlod is WRITTEN once by its lane - with an order that is row order[pos] -,
 *      never added to and touched by no atomic, whatever NIC_HASH_FUSED_ADD_GRADS says; nothing past n_points is touched, and a call with
 *      n_points == 0 touches nothing.
 *      nic_hash_fused_forward_backward_points_grad_lod is nic_hash_fused_forward_backward_points_grad, argument for argument, with dlod
 *      [n_points] after dpoints and a level of detail always on: lodp == NULL and dlod == NULL are NIC_E_NULL among the pointers.  Everything
 *      else is the sibling's called with the same nic_hash_lod: the same two launches, records, fixed-order reduction, flags, tail,
 *      nic_mark_kernel_end, workspace (nic_hash_fused_points_workspace_bytes), noise, loss, y, decoder gradients and table gradient;
 *      table_grad == NULL (a frozen table) still produces dpoints, dlod and the decoder records; dpoints is the sibling's bit for bit, and
 *      without noise dlod is nic_hash_fused_points_grad_lod's with target on the same table bit for bit.
 *      Host checks, all before any GPU work, in the sibling's order with its codes: null desc / mlp (NIC_E_NULL); the fused set
 *      (nic_hash_fused_supported's code); the descriptor of a point source (NIC_E_SHAPE / NIC_E_ARG); null lodp, table, points, decoder
 *      layer, target, mlp_grads, loss, dpoints, dlod or workspace (NIC_E_NULL; quant, lod, order, table_grad, y and tail may be null); flags
 *      (NIC_E_ARG); the nic_hash_lod (NIC_E_ARG); quant (num_bits 1 .. 8, sample_base >= 0, noise_mode: NIC_E_ARG; NIC_NOISE_TENSOR is
 *      NIC_E_UNSUPPORTED); n_points < 0, or >= 2^31 with an order (NIC_E_ARG); the workspace (NIC_E_WORKSPACE); the tail (its codes);
 *      n_points == 0 is NIC_OK with nothing written.
 *      nic_hash_encode_points_grad_lod_noisy is the layer-wise sibling for the fp32 table, since training reads nothing else:
 *      nic_hash_encode_points_grad_lod from `table` [L, T, F] fp32 with a NULLABLE nic_hash_quant checked as the training entries check it.
 *      With quant == NULL or noise_mode NIC_NOISE_NONE its dpoints and dlod are nic_hash_encode_points_grad_lod's from an fp32 source bit
 *      for bit; with NIC_NOISE_KERNEL dpoints stays that (noise is a constant of the positions) and dlod gains the nz term.  One launch, no
 *      atomics, the same call gives the same bits.
 *      Host checks: the descriptor of a point source; null lodp, table, points, dx, dpoints or dlod (NIC_E_NULL; quant and lod may be
 *      null); the nic_hash_lod (NIC_E_ARG); quant (as above); n_points < 0 (NIC_E_ARG); n_points == 0 is NIC_OK without a launch.
 *      The batched form is the section below.  There is no bit depth per level, no 16-bit precision mode, no stored table, no second derivative and no gradient
 *      with respect to fade. */
int nic_hash_encode_points_grad_lod_noisy(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_quant *quant, const float *table,
                                          const float *points, const float *lod, int64_t n_points, const float *dx, float *dpoints,
                                          float *dlod, void *stream);
int nic_hash_fused_forward_backward_points_grad_lod(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_quant *quant,
                                                    const float *table, const float *points, const float *lod, int64_t n_points,
                                                    const int32_t *order, const nic_mlp *mlp, const float *target, float loss_scale,
                                                    float *table_grad, const nic_mlp_grads *mlp_grads, float *loss, float *y, float *dpoints,
                                                    float *dlod, int flags, void *workspace, size_t workspace_bytes,
                                                    const nic_step_tail *tail, void *stream);

/* ---- B hash-grid fields per launch with the gradient with respect to the LEVEL OF DETAIL, alone and in the training step (hashgrid.py,
 *      hash_batch_points_grad_lod, hash_batch_forward_backward_points_grad_lod, HashGridFieldBatch.point_gradient_lod / jacobian_lod /
 *      query_differentiable_lod / train_points_grad_lod / train_points_differentiable_lod; csrc/hashgrid_batch_grad.hip,
 *      hash_batch_points_grad_kernel<.., DLOD>; csrc/hashgrid_batch.hip, hash_batch_points_joint_lod_kernel).
 *      nic_hash_batch_points_grad_lod is nic_hash_batch_points_grad and nic_hash_batch_forward_backward_points_grad_lod is
 *      nic_hash_batch_forward_backward_points_grad, argument for argument, with dlod after dpoints and a level of detail always on: the
 *      same launches, gathers, records, reduction, flags, workspace, counts and order; y and dpoints (and loss and the decoder gradients
 *      of the step) are the siblings' called with the same nic_hash_lod bit for bit.  dlod = [B, n_points] fp32 on the device; the
 *      definitions are the two sections above, per field: dlod[b, n] = passes ? - sum_{l on the ramp} sum_f g[l F + f] (r[l, f] + nz[l F + f])
 *      : 0 with lambda_raw = (lod ? lod[b, n] : 0) + lod_uniform read at the field-local ROW n, g = d loss_b / d row (with target the
 *      output gradient is 2 (y - target) loss_scale / (3 n_b), n_b the field's OWN count), r the unweighed blend of field b's table at the
 *      rounded, clamped position, nz the noise the step's forward added - keyed by sample_base + n, n the field-local row whatever the
 *      order - and 0 in the gradient-only entry, which has no quant.  The right-hand derivative: a_raw == 1 has slope -1, a_raw == 0 slope 0;
 *      exactly 0.0f where lambda_raw < 0, >= 32 or NaN; a clamped axis zeroes its dpoints and not dlod.  Row order[b, pos] of dlod is
 *      WRITTEN once by the lane that handles it, never added to and touched by no atomic, whatever NIC_HASH_FUSED_ADD_GRADS says; rows at or
 *      past n_b, and rows an order does not name, are NOT written; a field with n_b = 0 writes nothing.  Field b's rows are
 *      nic_hash_fused_points_grad_lod's / nic_hash_fused_forward_backward_points_grad_lod's on field b's tensors bit for bit.  The gradient
 *      for lod_uniform, or for a lod shared by the fields, is a sum of dlod; the caller forms it.
 *      Host checks, all before any GPU work: the siblings' in the siblings' order with two changes - lodp == NULL is NIC_E_NULL, reported
 *      with the other pointers (these are _lod entries; lod may be null), and dlod == NULL is NIC_E_NULL in the same check; the
 *      nic_hash_lod is checked where the siblings check it.  n_points == 0 is NIC_OK without a launch, nothing written.
 *      There is no 16-bit precision mode, no bit depth per level, no second derivative and no gradient with respect to fade. */
int nic_hash_batch_points_grad_lod(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_hash_lod *lodp,
                                   const nic_hash_source *src, const float *points, const float *lod, int64_t n_points,
                                   const int32_t *counts, const int32_t *order, const nic_mlp *mlp, const float *dy,
                                   const float *target, float loss_scale, float *y, float *dpoints, float *dlod, void *stream);
int nic_hash_batch_forward_backward_points_grad_lod(const nic_hash_desc *desc, int n_fields, int groups_per_field,
                                                    const nic_hash_lod *lodp, const nic_hash_quant *quant, const float *tables,
                                                    const float *points, const float *lod, int64_t n_points, const int32_t *counts,
                                                    const int32_t *order, const nic_mlp *mlp, const float *target, float loss_scale,
                                                    float *table_grads, const nic_mlp_grads *mlp_grads, float *loss, float *y, float *dpoints,
                                                    float *dlod, int flags, void *workspace, size_t workspace_bytes, void *stream);

/* ---- The training step at points with a WEIGHT PER POINT in its loss (hashgrid.py, hash_fused_forward_backward_points_weighted,
 *      HashGridField.train_points_weighted / train_points_weighted_differentiable / fit_points_weighted / fit_mips_weighted;
 *      csrc/hashgrid_weighted.hip, hash_points_weighted_train_kernel).
 *      weight = NULL, or [n_points] fp32 on the device, read at the row the point is read at (order[pos] clamped with an order, as target and
 *      lod are).  w_n = weight[n] > 0 ? weight[n] : 0: a NaN and a negative value count 0; +inf is the caller's error - no fault, the results
 *      are undefined.  weight == NULL is w = 1.
 *          loss = loss_scale sum_n w_n sum_o (y[n, o] - target[n, o])^2 / (3 n_points)
 *      - n_points, not sum w: ones give the plain loss, importance weights 1 / (N p_n) go in as they are, and a caller who wants the weighted
 *      mean divides the weights by their mean.  Every gradient is the derivative of that loss: d loss / d row of point n carries w_n, and so
 *      do the table gradient, the decoder gradients, dpoints[n] and dlod[n] (the conventions of the two sections above unchanged: the
 *      right-hand derivative, -(r + nz) on the ramp under noise, exactly 0.0f where lambda is clamped or NaN, a clamped axis zeroes its
 *      dpoints).  A point of weight 0 still gets its y, adds exactly +0 to the loss, gets dpoints / dlod == 0.0f and adds zeros to every
 *      gradient: a table entry only such points touch keeps its value.
 *      The call is nic_hash_fused_forward_backward_points_grad_lod with `weight` after lod, and lodp, dpoints and dlod NULLABLE: without lodp
 *      there is no level of detail (the plain rows, bit for bit), without dpoints no second walk of the levels, without dlod no lambda
 *      accumulator.  Everything else is the siblings': the same two launches, records, fixed-order reduction, flags, tail,
 *      nic_mark_kernel_end, workspace (nic_hash_fused_points_workspace_bytes), noise keys (sample_base + row); table_grad == NULL is a frozen
 *      table, everything else is still produced.  With weight == NULL, or all ones, loss, y, the six decoder gradients, dpoints and dlod are
 *      bit for bit those of the sibling that takes the remaining arguments (nic_hash_fused_forward_backward_points, _points_lod,
 *      _points_grad, _points_grad_lod), and the table gradient agrees with it as two calls of that sibling agree (the order of the atomics).
 *      Host checks, all before any GPU work, in this order: null desc / mlp (NIC_E_NULL); the fused set (nic_hash_fused_supported's code);
 *      the descriptor of a point source (NIC_E_SHAPE / NIC_E_ARG); null table, points, decoder layer, target, mlp_grads, loss or workspace
 *      (NIC_E_NULL; lodp, quant, lod, weight, order, table_grad, y, dpoints, dlod and tail may be null); flags (NIC_E_ARG); lod without
 *      lodp, dlod without lodp, dlod without dpoints (NIC_E_ARG); the nic_hash_lod where given (NIC_E_ARG); quant (num_bits 1 .. 8,
 *      sample_base >= 0, noise_mode: NIC_E_ARG; NIC_NOISE_TENSOR is NIC_E_UNSUPPORTED); n_points < 0, or >= 2^31 with an order (NIC_E_ARG);
 *      the workspace (NIC_E_WORKSPACE); the tail (its codes); n_points == 0 is NIC_OK with nothing written.
 *      There are no weights on the batched entries (their ragged counts are the 0 / 1 case), none on the crop route, none per channel, no
 *      bit depth per level and no 16-bit precision mode. */
int nic_hash_fused_forward_backward_points_weighted(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_quant *quant,
                                                    const float *table, const float *points, const float *lod, const float *weight,
                                                    int64_t n_points, const int32_t *order, const nic_mlp *mlp, const float *target,
                                                    float loss_scale, float *table_grad, const nic_mlp_grads *mlp_grads, float *loss, float *y,
                                                    float *dpoints, float *dlod, int flags, void *workspace, size_t workspace_bytes,
                                                    const nic_step_tail *tail, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NICV2_HIP_EXT_H */
