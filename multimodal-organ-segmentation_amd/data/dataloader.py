"""get_dataloader(config, split) — reference src/data/dataloader.py:14-60.

Without data.synthetic the loader reads the reference's CSV lists of NIfTI files
(data_root/{train_csv, val_csv, test_csv}) and decodes, normalises, augments and
resizes them on the GPU (data/nifti.py).  With data.synthetic it serves the seeded
phantoms of data/synthetic.py in the same batch format.  Under data parallelism each rank takes samples r, r+W, ...
(DistributedSampler semantics).  With data.synthetic.device: true
the phantoms are generated and normalised on the GPU instead (data/device.py), and
data.augmentation.enabled: true augments the training split there (data/augment.py).  data.patch.enabled: true
trains on patches drawn from the volumes at their own size and validates on the full-size volumes
(data/patch.py); with the key absent or false nothing changes."""
from typing import Any, Dict

import torch
from torch.utils.data import DataLoader, Subset

from ..distributed import ddp
from .synthetic import SyntheticSegDataset


def get_dataset(config: Dict[str, Any], split: str = "train"):
    syn = config["data"].get("synthetic")
    if syn is None:
        # data_root/{train,val,test}_csv of NIfTI files, decoded and transformed on the GPU (data/nifti.py);
        # no GPU is touched before the first sample is fetched
        from .augment import DeviceAugment
        from .nifti import DeviceNiftiDataset, read_data_list
        aug_cfg = config["data"].get("augmentation") or {}
        augment = DeviceAugment(aug_cfg) if split == "train" and aug_cfg.get("enabled", False) else None
        return DeviceNiftiDataset(config, read_data_list(config, split), mode=split, augment=augment)
    n = syn["n_train"] if split == "train" else syn.get("n_val", 2)
    seed = syn.get("seed", 1234) + (0 if split == "train" else 100000)
    return SyntheticSegDataset(n, syn.get("size", 96), config["model"]["out_channels"], config["data"]["modalities"],
                               seed=seed)


def _patch_dataloader(config: Dict[str, Any], patch_cfg: Dict[str, Any], split: str, shuffle):
    """data.patch.enabled: the training split draws patches from volumes at their own size (data/patch.py); val /
    test yield the full-size volumes one by one, for the sliding windows of Trainer._validate."""
    from .augment import DeviceAugment
    from .device import DeviceLoader, DevicePhantomDataset
    from .patch import DevicePatchDataset, PatchLoader
    syn = config["data"].get("synthetic")
    if syn is None:
        from .nifti import DeviceNiftiDataset, read_data_list
        ds = DeviceNiftiDataset(config, read_data_list(config, split), mode=split, resize=False)
    elif syn.get("device", False):
        n = syn["n_train"] if split == "train" else syn.get("n_val", 2)
        seed = syn.get("seed", 1234) + (0 if split == "train" else 100000)
        ds = DevicePhantomDataset(n, syn.get("size", 96), config["model"]["out_channels"],
                                  config["data"]["modalities"], torch.device("cuda", torch.cuda.current_device()),
                                  seed=seed, preprocessing=config["data"].get("preprocessing"))
    else:
        raise NotImplementedError("data.patch.enabled needs the device data path: NIfTI lists or "
                                  "data.synthetic.device: true (the sampler is a HIP pass, there is no CPU path)")
    if split != "train":
        return DeviceLoader(ds, 1, shuffle=False if shuffle is None else shuffle, drop_last=False, seed=ds.seed,
                            pad=False)
    aug_cfg = config["data"].get("augmentation") or {}
    augment = DeviceAugment(aug_cfg) if aug_cfg.get("enabled", False) else None
    return PatchLoader(DevicePatchDataset(ds, patch_cfg, augment=augment), config["training"]["batch_size"],
                       shuffle=True if shuffle is None else shuffle, seed=ds.seed)


def get_dataloader(config: Dict[str, Any], split: str = "train", shuffle=None, drop_last=None):
    patch_cfg = config["data"].get("patch")
    if patch_cfg is not None:
        from .patch import patch_config
        if patch_config(patch_cfg)["enabled"]:
            return _patch_dataloader(config, patch_cfg, split, shuffle)
    if config["data"].get("synthetic") is None:
        from .device import DeviceLoader
        ds = get_dataset(config, split)
        return DeviceLoader(ds, config["training"]["batch_size"],
                            shuffle=split == "train" if shuffle is None else shuffle,
                            drop_last=split == "train" if drop_last is None else drop_last, seed=ds.seed,
                            pad=split == "train")
    syn = config["data"].get("synthetic") or {}
    aug_cfg = config["data"].get("augmentation") or {}
    augment = split == "train" and aug_cfg.get("enabled", False)    # get_transforms: the train pipeline only
    if syn.get("device", False):
        # data.synthetic.device: true -> phantoms generated and normalised on the GPU (data/device.py)
        from .augment import DeviceAugment
        from .device import DeviceLoader, DevicePhantomDataset
        n = syn["n_train"] if split == "train" else syn.get("n_val", 2)
        seed = syn.get("seed", 1234) + (0 if split == "train" else 100000)
        ds = DevicePhantomDataset(n, syn.get("size", 96), config["model"]["out_channels"],
                                  config["data"]["modalities"], torch.device("cuda", torch.cuda.current_device()),
                                  seed=seed, preprocessing=config["data"].get("preprocessing"),
                                  augment=DeviceAugment(aug_cfg) if augment else None)
        return DeviceLoader(ds, config["training"]["batch_size"],
                            shuffle=split == "train" if shuffle is None else shuffle,
                            drop_last=split == "train" if drop_last is None else drop_last, seed=seed,
                            pad=split == "train")
    if augment:
        raise NotImplementedError("data.augmentation.enabled needs the device data path: set "
                                  "data.synthetic.device: true (augmentation is a HIP pass, there is no CPU path)")
    ds = get_dataset(config, split)
    w, r = ddp.world(), ddp.rank()
    if w > 1:   # training shards are padded to equal length, validation shards are not (each sample once)
        ds = Subset(ds, ddp.shard_indices(len(ds), r, w, pad=split == "train"))
    if shuffle is None:
        shuffle = split == "train"
    if drop_last is None:
        drop_last = split == "train"
    hw = config.get("hardware", {})
    nw = hw.get("num_workers", 0)
    return DataLoader(ds, batch_size=config["training"]["batch_size"], shuffle=shuffle, num_workers=nw,
                      pin_memory=hw.get("pin_memory", True) and torch.cuda.is_available(), drop_last=drop_last,
                      persistent_workers=nw > 0)
