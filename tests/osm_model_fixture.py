"""Shared by the OSMObjESRGANModel tests: the loader of tests/golden/osm_model_aa{0,1}_*.pt (tools/make_osm_model_golden.py) and the
option dictionary that drives the model through the recorded step.  (Not a test module.)"""
import glob
import os
from collections import OrderedDict

import torch

import osm_disc_fixture as fx

GOLDEN = fx.GOLDEN
OSM_MINI = os.path.join(GOLDEN, "osm_mini", "osm_chips_to_masks.json")


def load(aa: int):
    """the head of run `aa` (0: antialias off, 1: on) with the piece files reassembled: g_grads, d_grads, g_final, d_final, and d0, the
    discriminator's full initial state (the ruled object branch, then the stored U-Net half)"""
    name = f"osm_model_aa{aa}"
    head = torch.load(os.path.join(GOLDEN, name + "_head.pt"), weights_only=False)
    parts = {}
    for f in sorted(glob.glob(os.path.join(GOLDEN, name + "_part_*.pt"))):
        for (tag, key, j), t in torch.load(f, weights_only=False).items():
            parts.setdefault((tag, key), {})[j] = t
    for (tag, key), shape in head["shapes"].items():
        p = parts[(tag, key)]
        head.setdefault(tag, OrderedDict())[key] = torch.cat([p[j] for j in range(len(p))]).reshape(shape)
    d0 = fx.object_branch_state(head["trial"])
    d0.update(head["unet0"])
    head["d0"] = d0
    return head


def batch_of(head):
    return {"lr": head["lr_u8"], "hr": head["hr_u8"], "Phase": ["train"] * head["lr_u8"].shape[0], "Chip": list(head["chip_names"])}


def boxes_of(head):
    """(b, x1, y1, x2, y2) of the chosen objects, resolved by the project's own host code"""
    from satlas_super_resolution_amd import osm_reference as R
    H, W = head["hr_u8"].shape[-2:]
    out = []
    for b, (chip, idx) in enumerate(zip(head["chip_names"], head["chosen"])):
        res = R.resolve_boxes(R.flatten_objects(head["chips"][chip]), H, W, chip)
        out += [(b,) + res[i] for i in idx]
    return out


def model_opt(head, tmp, mode="fp32", deterministic=False):
    """the option dictionary of the recorded step; the initial networks and the chips file are written under `tmp`"""
    import json
    g_path, d_path, j_path = (os.path.join(str(tmp), n) for n in ("g0.pth", "d0.pth", "osm_chips_to_masks.json"))
    torch.save({"params": head["g0"]}, g_path)
    torch.save({"params": head["d0"]}, d_path)
    with open(j_path, "w") as f:
        json.dump(head["chips"], f)
    adam = lambda: {"type": "Adam", "lr": head["lr"], "weight_decay": 0, "betas": list(head["betas"])}
    return dict(is_train=True, model_type="OSMObjESRGANModel", scale=4, manual_seed=0, compute_dtype=mode, deterministic=deterministic,
                network_g=dict(type="SSR_RRDBNet", **head["g_kwargs"]), network_d=dict(type="OSMObjDiscriminator", **head["d_kwargs"]),
                osm_obj_weight=head["osm_obj_weight"], osm_obj_resize_antialias=head["antialias"], **head["opt"],
                datasets=dict(train=dict(osm_objs_path=j_path, n_osm_objs=head["n_osm_objs"])),
                path=dict(pretrain_network_g=g_path, param_key_g="params", pretrain_network_d=d_path, param_key_d="params",
                          models=os.path.join(str(tmp), "models"), training_states=os.path.join(str(tmp), "states")),
                train=dict(ema_decay=head["ema_decay"], optim_g=adam(), optim_d=adam(), net_d_iters=1, net_d_init_iters=0,
                           pixel_opt=dict(type="L1Loss", loss_weight=head["l1_weight"], reduction="mean"),
                           gan_opt=dict(type="GANLoss", gan_type="vanilla", real_label_val=1.0, fake_label_val=0.0, loss_weight=head["gan_weight"])))
