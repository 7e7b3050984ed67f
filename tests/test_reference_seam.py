"""The seam between the reference's driver code and this package: BasicSR's registries resolving our classes.

`ssr/train.py:62` calls `basicsr.models.build_model(opt)`, which looks `opt['model_type']` up in BasicSR's MODEL_REGISTRY; the model
then calls `basicsr.archs.build_network(opt['network_g'])` (ARCH_REGISTRY).  satlas_super_resolution_amd/registry.py registers the HIP
classes into THOSE registries when BasicSR is importable.  BasicSR (requirements.txt:1, basicsr==1.4.2) does not travel with this
repo: where it is installed the test uses it, elsewhere a stand-in package of the same shape (`basicsr.utils.registry` with the three
registries, `basicsr.archs.build_network`, `basicsr.models.build_model`, written to the test's temporary directory).  The body runs
in a fresh interpreter, so that registry.py binds to those registries when it is first imported.  The two sides of the seam are also
pinned separately: our registry / model plugin against the unmodified `optimize_parameters` (tests/test_gpu_boundary.py), the key
layout against the reference modules' state_dicts (tests/test_host_boundary.py)."""
import importlib.util
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the parts of BasicSR 1.4.2 the seam touches, same names and call shapes.  Written out here on purpose, independent of
# satlas_super_resolution_amd/registry.py (whose fallback Registry looks alike): the stand-in plays BasicSR, the side the
# code under test must bind to, so it must not share code with it.
STANDIN = {
    "basicsr/__init__.py": "",
    "basicsr/utils/__init__.py": "",
    "basicsr/utils/registry.py": '''
        class Registry:
            def __init__(self, name):
                self._name, self._obj_map = name, {}

            def _do_register(self, name, obj, suffix=None):
                if isinstance(suffix, str):
                    name = name + "_" + suffix
                assert name not in self._obj_map, f"{name} already registered in {self._name}"
                self._obj_map[name] = obj

            def register(self, obj=None, suffix=None):
                if obj is None:
                    def deco(func_or_class):
                        self._do_register(func_or_class.__name__, func_or_class, suffix)
                        return func_or_class
                    return deco
                self._do_register(obj.__name__, obj, suffix)

            def get(self, name, suffix="basicsr"):
                ret = self._obj_map.get(name, self._obj_map.get(name + "_" + suffix))
                if ret is None:
                    raise KeyError(f"No object named '{name}' found in '{self._name}' registry!")
                return ret

            def __contains__(self, name):
                return name in self._obj_map

            def keys(self):
                return self._obj_map.keys()


        DATASET_REGISTRY = Registry("dataset")
        ARCH_REGISTRY = Registry("arch")
        MODEL_REGISTRY = Registry("model")
        ''',
    "basicsr/archs/__init__.py": '''
        from copy import deepcopy
        from basicsr.utils.registry import ARCH_REGISTRY


        def build_network(opt):
            opt = deepcopy(opt)
            return ARCH_REGISTRY.get(opt.pop("type"))(**opt)
        ''',
    "basicsr/models/__init__.py": '''
        from copy import deepcopy
        from basicsr.utils.registry import MODEL_REGISTRY


        def build_model(opt):
            opt = deepcopy(opt)
            return MODEL_REGISTRY.get(opt["model_type"])(opt)
        ''',
}

BODY = '''
import sys
import torch
import basicsr.utils.registry as R
import satlas_super_resolution_amd.archs  # noqa: F401  (registers SSR_RRDBNet / SSR_UNetDiscriminatorSN in BasicSR's ARCH_REGISTRY)
import satlas_super_resolution_amd.models  # noqa: F401  (SSRESRGANModel in MODEL_REGISTRY)
from basicsr.archs import build_network        # what ssr_esrgan_model.py:43,53 call
from basicsr.models import build_model         # what ssr/train.py:62 calls
from satlas_super_resolution_amd import registry
from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
from satlas_super_resolution_amd.archs.discriminator_arch import SSR_UNetDiscriminatorSN
from satlas_super_resolution_amd.models.ssr_esrgan_model import SSRESRGANModel
from satlas_super_resolution_amd.utils.model_utils import build_network as build_infer
assert registry.ARCH_REGISTRY is R.ARCH_REGISTRY and registry.MODEL_REGISTRY is R.MODEL_REGISTRY, "registry.py did not bind to BasicSR"
assert R.ARCH_REGISTRY.get("SSR_RRDBNet") is SSR_RRDBNet and R.ARCH_REGISTRY.get("SSR_UNetDiscriminatorSN") is SSR_UNetDiscriminatorSN
assert R.MODEL_REGISTRY.get("SSRESRGANModel") is SSRESRGANModel
net = build_network({"type": "SSR_RRDBNet", "num_in_ch": 24, "num_out_ch": 3, "num_feat": 64, "num_block": 1, "num_grow_ch": 32})
assert isinstance(net, SSR_RRDBNet)
model = build_model(OPT)
assert isinstance(model, SSRESRGANModel)
torch.manual_seed(0)
for it in (1, 2):                              # the loop body of ssr/train.py:106-110
    model.update_learning_rate(it, warmup_iter=-1)
    model.feed_data({"lr": torch.randint(0, 256, (2, 24, 32, 32), dtype=torch.uint8), "hr": torch.randint(0, 256, (2, 3, 128, 128), dtype=torch.uint8)})
    model.optimize_parameters(it)
log = model.get_current_log()
assert {"l_g_pix", "l_g_gan", "l_d_real", "l_d_fake"} <= set(log) and all(v == v for v in log.values()), log
# the reference's inference helper with the reference's own import line swapped (INTEGRATION.md section 1)
g = build_infer({"n_lr_images": 8, "network_g": {"type": "SSR_RRDBNet", "num_in_ch": 24, "num_out_ch": 3, "num_feat": 64, "num_block": 1, "num_grow_ch": 32}})
assert isinstance(g, SSR_RRDBNet)
print("SEAM OK", "installed BasicSR" if not R.__file__.startswith(STANDIN_DIR) else "stand-in BasicSR")
'''


def _opt(tmp_path):
    return {
        "name": "seam", "model_type": "SSRESRGANModel", "scale": 4, "num_gpu": 1, "manual_seed": 0, "is_train": True, "dist": False,
        "rank": 0, "world_size": 1, "l1_gt_usm": False, "percep_gt_usm": False, "gan_gt_usm": False, "feed_disc_lr": False,
        "network_g": {"type": "SSR_RRDBNet", "num_in_ch": 24, "num_out_ch": 3, "num_feat": 64, "num_block": 1, "num_grow_ch": 32},
        "network_d": {"type": "SSR_UNetDiscriminatorSN", "num_in_ch": 3, "num_feat": 64, "skip_connection": True},
        "path": {"pretrain_network_g": None, "models": str(tmp_path / "models"), "training_states": str(tmp_path / "states"),
                 "visualization": str(tmp_path / "vis"), "experiments_root": str(tmp_path), "log": str(tmp_path)},
        "train": {"ema_decay": 0.999, "optim_g": {"type": "Adam", "lr": 1e-4, "weight_decay": 0, "betas": [0.9, 0.99]},
                  "optim_d": {"type": "Adam", "lr": 1e-4, "weight_decay": 0, "betas": [0.9, 0.99]},
                  "scheduler": {"type": "MultiStepLR", "milestones": [400000], "gamma": 0.5}, "total_iter": 2, "warmup_iter": -1,
                  "pixel_opt": {"type": "L1Loss", "loss_weight": 1.0, "reduction": "mean"},
                  "gan_opt": {"type": "GANLoss", "gan_type": "vanilla", "real_label_val": 1.0, "fake_label_val": 0.0, "loss_weight": 0.1},
                  "net_d_iters": 1, "net_d_init_iters": 0},
        "logger": {"print_freq": 1, "save_checkpoint_freq": 100},
    }


def test_basicsr_build_model_resolves_the_hip_plugin_and_trains(tmp_path):
    standin = tmp_path / "standin"
    if importlib.util.find_spec("basicsr") is None:
        for rel, text in STANDIN.items():
            (standin / rel).parent.mkdir(parents=True, exist_ok=True)
            (standin / rel).write_text(textwrap.dedent(text).lstrip())
    script = tmp_path / "seam.py"
    script.write_text(f"OPT = {_opt(tmp_path)!r}\nSTANDIN_DIR = {str(standin)!r}\n" + BODY)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(standin), ROOT] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
    r = subprocess.run([sys.executable, str(script)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "SEAM OK" in r.stdout, r.stdout[-2000:]
    print(r.stdout.strip().splitlines()[-1])
