"""Host-side mirror of the reference's data/ package (data_utils.py, dataloader.py: same names and argument order) with
the clouds resident on the device and the per-batch work in one HIP kernel (sug_prepare_batch; sug_prepare_batch_aug with the scale, rotation-perturbation and shift stages), and the part-segmentation dataset on the same plan (partseg.py:
sug_prepare_seg_batch)."""
from .partseg import PartSegDataset, pack_clouds  # noqa: F401
