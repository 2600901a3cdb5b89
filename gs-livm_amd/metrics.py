"""Host-side mirror of the reference's evaluation pass on the fused kernels of csrc/metrics.hip: what saveRender
(src/liw/lioOptimization.cpp:2182-2245) and the status line of optimize_vis (:1739-1776) run on the device around a
forward-only render -- gaussian_splatting::psnr and ::ssim (include/gs/gs/loss_utils.cuh:89-93, 43-70) and the 8-bit
images of tensor2CvMat3X (:2113-2136) and tensor2CvMat2X (:2150-2164).  The JET colour map, PNG and MP4 writing stay
with the host application."""
import torch

from . import _capi
from .loss import apply_exposure, reference_window_1d
from .render_utils import render


def image_metrics(img, gt, window11=None, totals=None, weights=None):
    """-> device tensor [psnr, ssim, l1, mse] of img against gt ([C,H,W] f32 on the device), two launches, no host
    round trip.  psnr is the reference's mean of the per-channel PSNRs (+inf where a channel is identical); ssim and l1
    are those of `photometric_loss`.  totals: a device float64 [4] that {psnr, ssim, l1, 1} is added to (the running
    sums and the frame count of a keyframe sweep).  weights: [H,W] f32 on the device, finite and >= 0 (an undistortion
    border, a sky mask): the four numbers are then those of `weighted_photometric_loss` -- every sum weighted per pixel
    and divided by the weight sum -- so that pixels without a measurement are not charged."""
    if window11 is None:
        window11 = reference_window_1d()
    if weights is None:
        return _capi.image_metrics(img, gt, window11.tolist(), totals=totals)
    return _weighted_metrics(img, gt, weights, window11.tolist(), None, totals)


def _weighted_metrics(img, gt, weights, win, out, totals):
    """{psnr, ssim, l1, mse} from the forward and finish of csrc/weighted.hip; `totals` as image_metrics adds to it."""
    with torch.no_grad():
        H, W = int(img.shape[1]), int(img.shape[2])
        out6, _, _ = _capi.weighted_loss(img.detach(), gt.detach(), weights.detach().reshape(H, W), None, 0.0, None, win,
                                         0.0, want_grad=False)
        row = out6[[5, 2, 1, 4]]
        if out is not None:
            out.copy_(row)
            row = out
        if totals is not None:
            totals[:3] += row[:3].double()
            totals[3] += 1.0
    return row


def psnr(img, gt):
    """Drop-in for gaussian_splatting::psnr(rendered_img, gt_img) (loss_utils.cuh:89-93): a 0-dim device tensor."""
    return image_metrics(img, gt)[0]


def to_u8(img, bgr=True, out=None):
    """tensor2CvMat3X (:2113-2136) on the device: [3,H,W] f32 -> uint8 [H,W,3], x * 255 clamped to [0, 255] and
    truncated (NaN -> 0), channels swapped for cv::imwrite unless bgr=False.  out: a uint8 [H,W,3] view to write into
    -- e.g. a column slice of a wider [H,2W,3] image -- whose bytes outside the written pixels are left alone."""
    return _capi.pack_image_u8(img, bgr=bgr, out=out)


def side_by_side(img, gt, bgr=True):
    """cv::hconcat(render_image, gt_image) of saveRender (:2219-2220): one uint8 [H,2W,3] device image."""
    H, W = int(img.size(1)), int(img.size(2))
    both = torch.empty((H, 2 * W, 3), dtype=torch.uint8, device=img.device)
    to_u8(img, bgr=bgr, out=both[:, :W])
    to_u8(gt, bgr=bgr, out=both[:, W:])
    return both


def depth_to_u8(depth, max_depth=50.0, out=None):
    """tensor2CvMat2X (:2150-2164) up to its colour map: [H,W] or [1,H,W] f32 -> uint8 [H,W],
    round_half_even(depth * (255 / max_depth)) saturated to [0, 255] (NaN -> 0): cv::Mat::convertTo(CV_8U) as OpenCV
    documents it.  cv::applyColorMap(COLORMAP_JET) is the host's."""
    return _capi.pack_depth_u8(depth, max_depth, out=out)


def evaluate_keyframes(cameras, gts, model, bg, on_frame=None, window11=None, exposures=None, weights=None,
                       lidar_depths=None, acc_min=0.5):
    """The loop of saveRender (:2198-2231): every keyframe is rendered forward-only and measured against its ground
    truth ([3,H,W] f32 on the device); the per-frame metrics and their running float64 sums stay on the device and are
    copied to the host ONCE, after the last frame (the reference makes two .item() round trips per frame).
    on_frame(i, image, depth): hook of a host that exports frames (to_u8 / side_by_side / depth_to_u8, PNG writing).
    exposures: one learnt exposure per keyframe ([C,2] or [2], `exposure_photometric_loss`) or None for a keyframe
    without one; the render is compensated in place (`apply_exposure`) before it is measured and handed to on_frame,
    so that the metrics are not charged for the camera's gain.
    weights: one [H,W] weight map per keyframe (`image_metrics`' weights) or None for a keyframe measured on all pixels.
    lidar_depths: one [H,W] LiDAR depth image (`lidar_depth_image`, filtered or not) per keyframe or None for a
    keyframe without one; the render's depth is measured against it forward-only (the plain masked L1 of
    gsr_lidar_depth_loss_robust at lambda = 1, silhouette threshold acc_min) into a row of the same result buffer.
    -> dict(rows = CPU f32 [n,4] of {psnr, ssim, l1, mse} per frame, totals = CPU f64 [4] = {sum psnr, sum ssim,
    sum l1, n}, mean_psnr, mean_ssim, frames = n); with lidar_depths also depth_rows = CPU f32 [n,4] of {mean |depth
    error| in metres, the same, supervised share, clipped share = 0} per frame (a NaN row for a keyframe without an
    image) and mean_depth_error = the mean of the per-frame errors over the keyframes with an image and at least one
    supervised pixel (NaN when there is none)."""
    cameras, gts = list(cameras), list(gts)
    if len(cameras) != len(gts):
        raise ValueError("one ground-truth image per camera")
    n = len(cameras)
    exposures = [None] * n if exposures is None else list(exposures)
    if len(exposures) != n:
        raise ValueError("one exposure (or None) per camera")
    weights = [None] * n if weights is None else list(weights)
    if len(weights) != n:
        raise ValueError("one weight map (or None) per camera")
    if lidar_depths is not None:
        lidar_depths = list(lidar_depths)
        if len(lidar_depths) != n:
            raise ValueError("one LiDAR depth image (or None) per camera")
    dev = model.Get_xyz().device
    win = (reference_window_1d() if window11 is None else window11).tolist()
    # one buffer, one copy: the four float64 totals in front (8-byte aligned), the n float32 rows behind them
    # (and, with LiDAR images, the n float32 depth rows behind those)
    buf = torch.zeros(32 + 16 * n * (1 if lidar_depths is None else 2), dtype=torch.uint8, device=dev)
    totals, rows = buf[:32].view(torch.float64), buf[32:32 + 16 * n].view(torch.float32).view(n, 4)
    if lidar_depths is not None:
        drows = buf[32 + 16 * n:].view(torch.float32).view(n, 4)
        drows.fill_(float("nan"))
    with torch.no_grad():
        for i, (cam, gt) in enumerate(zip(cameras, gts)):
            image, depth, acc = render(cam, model, bg)
            if exposures[i] is not None:
                image = apply_exposure(image, exposures[i], out=image if image.is_contiguous() else None)
            if weights[i] is None:
                _capi.image_metrics(image, gt, win, out=rows[i], totals=totals)
            else:
                _weighted_metrics(image, gt, weights[i], win, rows[i], totals)
            if lidar_depths is not None and lidar_depths[i] is not None:
                _capi.lidar_depth_loss_robust(depth.contiguous(), acc.contiguous(), lidar_depths[i].contiguous(),
                                              acc_min, 1.0, 0.0, 0.0, float("inf"), 0.0, want_grad_depth=False,
                                              want_grad_acc=False, out4=drows[i])
            if on_frame is not None:
                on_frame(i, image, depth)
    host = buf.cpu()
    totals, rows = host[:32].view(torch.float64).clone(), host[32:32 + 16 * n].view(torch.float32).view(n, 4).clone()
    count = float(totals[3])
    mean = lambda s: float(s) / count if n else float("nan")  # noqa: E731  (the reference divides by count all the same)
    result = dict(rows=rows, totals=totals, mean_psnr=mean(totals[0]), mean_ssim=mean(totals[1]), frames=n)
    if lidar_depths is not None:
        drows = host[32 + 16 * n:].view(torch.float32).view(n, 4).clone()
        seen = drows[:, 2] > 0          # (false for the NaN rows)
        result["depth_rows"] = drows
        result["mean_depth_error"] = float(drows[seen, 1].double().mean()) if bool(seen.any()) else float("nan")
    return result
