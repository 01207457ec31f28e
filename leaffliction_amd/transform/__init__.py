"""GPU side of the reference's srcs/transform filters that sit on the augmentation hot path."""
from .filters import (TransformConfig, analyze_color_regions, analyze_filter_batch, apply_analyze_filter,  # noqa: F401
                      apply_blur_filter, apply_brown_filter, apply_histogram_filter, apply_landmarks_filter, apply_mask_filter, apply_roi_filter, brown_filter_batch, create_inclusive_mask,
                      hist_figure_batch, hist_figure_texts, hist_summary, hsv_density_curves, hue_range_counts, landmarks_filter_batch, leaf_hsv_histograms, leaf_landmarks, load_config, make_mask, make_masks,
                      measure_leaves, measure_lesions, mosaic_batch, roi_filter_batch)
