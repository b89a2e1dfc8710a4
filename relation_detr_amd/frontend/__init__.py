"""What runs in front of the backbone: images -> padded batch, mask, sizes and prepared targets (frontend/images.py), and the training
augmentation in front of that (frontend/augment.py)."""
from .augment import DetrAugment, DetrChoice, detr_plan, sample_detr_choices, shortest_size, transform_targets
from .images import (MAX_DOWNSCALE, MAX_IMAGES, ImageBatch, ImagePreprocessor, batch_images, batched_size, check_boxes, prepare_targets,
                     resize_image, resized_size)

__all__ = ["ImageBatch", "ImagePreprocessor", "batch_images", "batched_size", "check_boxes", "prepare_targets", "resize_image",
           "resized_size", "MAX_IMAGES", "MAX_DOWNSCALE", "DetrAugment", "DetrChoice", "detr_plan", "sample_detr_choices", "shortest_size",
           "transform_targets"]
