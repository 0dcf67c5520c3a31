"""Connected components on the device — what the reference's dataset loop asks of cv2 at main.py:168-180 (and :217-229).

After the segmentation of a randomised pose the reference labels the mask "everything that is not the glottis" with
cv2.connectedComponentsWithStats and drops the sample when the segmentation is empty or the mask falls into more than two
pieces.  Here the label image stays on the device: one call of ffx_connected_components (include/ffx_labels.h)
in place of a 2 MB copy to the host per sample.  The numbering of the components is scipy.ndimage.label's (raster order of the
first pixel), not promised to be cv2's; the reference reads n_labels alone.
"""
import torch

from .. import ops


def connected_components_with_stats(image, connectivity=8, max_labels=256):
    """cv2.connectedComponentsWithStats(image, connectivity=...) for a 2-D bool / uint8 / int32 / int64 device image: foreground where
    image != 0 -> (n_labels, labels, stats, centroids), device tensors in cv2's order: n_labels a 0-d int32 (components + 1), labels
    [H, W] int32, stats [max_labels, 5] int32 (left, top, width, height, area; row 0 the background), centroids [max_labels, 2]
    float64.  Rows from n_labels on are zeros / NaN; components beyond max_labels keep their labels and lose only their rows."""
    c = ops.connected_components(image, connectivity=connectivity, max_labels=max_labels)
    return c.n_labels, c.labels, c.stats, c.centroids


def connected_components(image, connectivity=8):
    """cv2.connectedComponents(image, connectivity=...) -> (n_labels, labels)"""
    c = ops.connected_components(image, connectivity=connectivity, stats=False)
    return c.n_labels, c.labels


def accept_segmentation(seg, glottis_label=2, max_labels=3):
    """Whether the reference's dataset loop keeps a sample with the label image `seg` of get_segmentation_from_camera (main.py:168-180):
        seg.max() != 0  and  n_labels(seg != glottis_label, 8-connected) <= max_labels
    -> a 0-d bool device tensor; nothing is read on the host.  The reference builds its mask as seg[seg == 1] = 0; seg[seg == 2] = 1;
    1 - seg; astype(uint8): label 2 becomes 0 and labels 0 and 1 become 1, while a label >= 3 becomes 1 - label, which wraps to a
    non-zero byte (254 for 3): EVERY label other than 2 is foreground, and that is the mask labelled here, by passing the glottis' label
    as the background.  No label image and no statistics are produced: only the launches the count needs run."""
    n = ops.connected_components(seg, connectivity=8, background=glottis_label, labels=False, stats=False).n_labels
    return torch.logical_and(seg.max() != 0, n <= max_labels)
