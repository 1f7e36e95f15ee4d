"""Shim for utils/loss.py: iou_loss (what train.py:80-85 uses), structure_loss and wbce, argument order as there."""
from tramba_amd.train import iou_loss, structure_loss, wbce  # noqa: F401
