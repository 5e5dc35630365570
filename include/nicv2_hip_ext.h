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

#ifdef __cplusplus
}
#endif
#endif /* NICV2_HIP_EXT_H */
