/*
 * simpleicp_hip_device.h -- companion C ABI of libsimpleicp_hip.so: clouds that already live in device memory.
 *
 * A host that holds its clouds in GPU buffers (a torch tensor, a buffer of its own) registers them without
 * moving a coordinate over the host link: the clouds are read where they lie, the selection is made on the
 * device, and the transformed movable cloud is written to a device buffer.  This header includes
 * simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries have
 * SICP_DEVICE_VERSION of their own.  The conventions of simpleicp_hip.h hold, except where said below.
 *
 * The road of one run (what simpleicp_amd.run_tensors does; SimpleICP.run computes the same):
 *   sicp_cloud_upload_strided(FIX), sicp_cloud_upload_strided(MOV)
 *   [sicp_select_in_range(ctx, FIX, MOV, NULL, n_fix, H0, max_overlap_distance, mask)   mask: device, n_fix bytes]
 *   sicp_select_n_device(ctx, mask or NULL, n_fix, correspondences, sel, &Q)             sel: device, correspondences int64
 *   sicp_estimate_normals(ctx, FIX, sel, Q, neighbors, normals, planarity, NULL)         outputs: device
 *   sicp_icp_setup(ctx, sel, Q, normals, planarity)
 *   sicp_icp_run(...), sicp_icp_uncertainties, sicp_icp_get_state
 *   sicp_cloud_write_strided(ctx, MOV, H, out, dtype, row_stride, col_stride)
 *
 * Ordering: every entry below runs on the ctx's stream (sicp_ctx_stream) and is complete on return, like
 * the rest of the ABI.  Work the caller queued on other streams that writes an input buffer must be complete,
 * or the ctx's stream must have been made to wait for it, before the call.
 */
#ifndef SIMPLEICP_HIP_DEVICE_H
#define SIMPLEICP_HIP_DEVICE_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_cloud_upload_strided, sicp_select_n_device, sicp_select_positions, sicp_cloud_write_strided. */
#define SICP_DEVICE_VERSION 1

#define SICP_DT_F32 1      /* float  */
#define SICP_DT_F64 2      /* double */

int sicp_device_version(void);

/* Uploads n points from a strided (n, 3) view in DEVICE memory on the ctx's device: point i, coordinate a is
 * base[i * row_stride + a * col_stride] (strides in elements, >= 0; any 2-D torch view of shape (n, 3)).
 * float32 is widened to float64 exactly.  One pass (k_ingest) writes the slot's padded column-wise layout and
 * measures the bounding box and the largest norm, so the slot ends in exactly the state sicp_cloud_upload of the
 * widened rows leaves: same coordinates, padding, statistics, index_base, no grid yet.  A host pointer, or memory
 * of another device, is SICP_ERR_INVALID; a non-finite coordinate is refused as by sicp_cloud_upload (same code,
 * same message, the slot is empty). */
int sicp_cloud_upload_strided(sicp_ctx *ctx, int slot, const void *base, int dtype, int64_t n, int64_t row_stride,
                              int64_t col_stride, int64_t index_base);

/* The selection of SimpleICP.run on the device: the rows of the fixed cloud (n points) whose mask byte is
 * non-zero -- mask (device, n bytes) as sicp_select_in_range writes it with a device in_range_out; NULL = every
 * row -- are compacted in index order (m rows), and select_n_points(Q) picks from them (pointcloud.py:132-147):
 * all m rows when m <= Q, else the rows at positions round_half_even(linspace(0, m - 1, Q)) (numpy's formula,
 * see sicp_select_positions).  sel_out: device memory for Q int64; *q_out = rows picked (0 when m == 0). */
int sicp_select_n_device(sicp_ctx *ctx, const uint8_t *mask, int64_t n, int64_t Q, int64_t *sel_out, int64_t *q_out);

/* The positions sicp_select_n_device picks among m kept rows for Q (host memory, min(m, Q) entries; *count_out
 * = how many): np.round(np.linspace(0, m - 1, Q)) when m > Q, 0 .. m - 1 otherwise.  Needs no device. */
int sicp_select_positions(int64_t m, int64_t Q, int64_t *pos_out, int64_t *count_out);

/* The slot's points under H, contract (T), written to DEVICE memory (k_egress): point i, coordinate a goes to
 * out[i * row_stride + a * col_stride] in dtype (float32: round-to-nearest of the float64 result).  With
 * SICP_DT_F64 the values are bit-identical to sicp_cloud_transform followed by sicp_cloud_download.  The slot
 * itself is NOT transformed: it keeps its coordinates, statistics and grid.  The caller owns out and its size. */
int sicp_cloud_write_strided(sicp_ctx *ctx, int slot, const double H[16], void *out, int dtype, int64_t row_stride,
                             int64_t col_stride);

#ifdef __cplusplus
}
#endif

#endif
