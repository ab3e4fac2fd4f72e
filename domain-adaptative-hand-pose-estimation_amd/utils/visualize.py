"""Debug images of a training run: a normalised network input with the predicted and the labelled skeleton drawn over it (PIL's
ImageDraw, as ``KeypointDataset.visualize``)."""
import numpy as np

from mi355.augment import MEAN, STD

PRED_COLOUR, LABEL_COLOUR = (255, 40, 40), (40, 220, 40)


def denormalize(image):
    """(3, H, W) normalised fp32 -> (H, W, 3) uint8."""
    a = np.asarray(image, dtype=np.float64) * np.asarray(STD)[:, None, None] + np.asarray(MEAN)[:, None, None]
    return (np.clip(np.nan_to_num(a), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0)


def visualize(image, pred, label, filename, bones=None):
    """Save `image` ((3, H, W), normalised) with the skeletons of `pred` and `label` ((K, 2) image pixels; either may be None):
    the label in green underneath, the prediction in red on top."""
    from PIL import Image, ImageDraw
    if bones is None:
        from uda.model.loss import HAND_BONES as bones
    canvas = Image.fromarray(denormalize(image), 'RGB')
    draw = ImageDraw.Draw(canvas)
    for pts, colour in ((label, LABEL_COLOUR), (pred, PRED_COLOUR)):
        if pts is not None:
            _skeleton(draw, pts, colour, bones)
    canvas.save(filename)
    return filename


def _skeleton(draw, pts, colour, bones):
    pts = np.nan_to_num(np.asarray(pts, dtype=np.float64), nan=-1.0e4, posinf=1.0e4, neginf=-1.0e4)
    for a, b in bones:
        draw.line([tuple(int(v) for v in pts[a]), tuple(int(v) for v in pts[b])], fill=colour, width=1)
    for x, y in pts:
        draw.ellipse([int(x) - 1, int(y) - 1, int(x) + 1, int(y) + 1], outline=colour)


def overlay(frame, preds, filename, labels=None, bones=None):
    """Save the uint8 (H, W, 3) RGB `frame` with the skeleton of every hand in `preds` (a list of (K, 2) arrays, frame pixels) in
    red on top of those of `labels` (optional, likewise) in green: the per-frame picture of predict.py --overlay."""
    from PIL import Image, ImageDraw
    if bones is None:
        from uda.model.loss import HAND_BONES as bones
    canvas = Image.fromarray(np.ascontiguousarray(frame, dtype=np.uint8), 'RGB')
    draw = ImageDraw.Draw(canvas)
    for group, colour in ((labels, LABEL_COLOUR), (preds, PRED_COLOUR)):
        for pts in group or ():
            _skeleton(draw, pts, colour, bones)
    canvas.save(filename)
    return filename
