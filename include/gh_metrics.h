/*
 * gh_metrics.h — C-ABI of the image-quality scores: MSE, PSNR and SSIM of rendered views against their targets,
 * as the reference's test step computes them (infer_one_shot.py:527-554 calling Evaluator.compute_score,
 * evaluator.py:85-118). LPIPS is not computed here.
 *
 * Per view v, with images in [0,1]:
 *   1. pred is taken as 0 wherever bbox_mask[v] == 0 (all 3 channels; bbox_mask may be NULL = keep every pixel);
 *      gt is not masked. Neither input is written.
 *   2. mse = mean((pred - gt)^2) over the whole H x W x 3 image, psnr = -10 log10(mse) (+inf when mse == 0).
 *   3. (x, y, w, h) = the tightest box around the non-zero pixels of mask_at_box[v] (cv2.boundingRect; (0,0,0,0) when
 *      the mask is empty). SSIM sees only that crop.
 *   4. ssim = scikit-image 0.16 structural_similarity(pred_crop, gt_crop, multichannel=True) with its defaults: per
 *      channel, 7x7 uniform window, sample covariance (49/48), C1 = (0.01 R)^2, C2 = (0.03 R)^2, the mean of S over the
 *      (w-6)(h-6) pixels whose window lies inside the crop, then the mean over the channels. R = data_range: the
 *      reference's float images get R = 2 (skimage takes the range of a float dtype as (-1, 1)). ssim is NaN when
 *      w < 7 or h < 7 (where skimage raises).
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host
 * synchronisation, no allocation, HIP-graph capturable; GhStatus return codes. No float atomics: every partial goes
 * to a fixed workspace slot and is summed in a fixed order, so results are bitwise reproducible run to run.
 * The SSIM window moments are accumulated in double precision.
 */
#ifndef GH_METRICS_H
#define GH_METRICS_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `layout`: memory order of pred and gt, one bit each. Both default to (Nv,3,H,W); a set bit means (Nv,H,W,3). */
#define GH_METRICS_CHW 0u
#define GH_METRICS_PRED_HWC 1u
#define GH_METRICS_GT_HWC 2u
#define GH_METRICS_HWC (GH_METRICS_PRED_HWC | GH_METRICS_GT_HWC)

/* Bytes of workspace gh_image_scores needs for these sizes (0 for invalid sizes). Pure host arithmetic. */
size_t gh_image_scores_workspace(int n_views, int H, int W);

/*
 * pred, gt: float32 images in the order `layout` gives. mask_at_box: (Nv,H,W) uint8, non-zero = inside.
 * bbox_mask: (Nv,H,W) uint8 or NULL. data_range: R above (finite, > 0).
 * scores: double[3 * Nv] receiving mse[0..Nv), psnr[0..Nv), ssim[0..Nv) in that order.
 * bbox: int32[4 * Nv] receiving (x, y, w, h) per view. workspace: >= gh_image_scores_workspace(Nv, H, W) bytes, 16-byte
 * aligned. Three kernel launches on `hip_stream`.
 */
int gh_image_scores(const float* pred, const float* gt, const uint8_t* mask_at_box, const uint8_t* bbox_mask, int n_views,
                    int H, int W, unsigned layout, double data_range, double* scores, int32_t* bbox, void* workspace,
                    size_t ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_METRICS_H */
