"""Golden vectors of the reference's VAEGAN encoder (gan_models/vaegan/train.py:61-96 `Encoder.encode`): tests/golden/vaegan_enc.npz.

Run in its own process (the reference's `utils` module name collides with attack_models/utils.py), where the reference tree is present:
    python tests/golden/make_golden_vaegan_enc.py
Only outputs and the byte images are stored; the weights are regenerated from the seed (synth.vaegan_encoder_state_dict)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _refimport  # noqa: E402

spec = importlib.util.spec_from_file_location("gl_synth", os.path.join(ROOT, "gan-leaks_amd", "synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)

SEED, IMAGE_SEED, N = 778, 779, 8
Z_DIMS = (100, 3)


def main():
    vg = _refimport.load("gan_models/vaegan/train.py", "ref_vaegan_train")
    u8 = synth.vaegan_encoder_images(IMAGE_SEED, N)
    x32 = (2.0 * (u8.astype(np.float64) / 255.0) - 1.0).astype(np.float32)       # the library's 8-bit lattice (attack_models/utils.py:82)
    out = {"images_u8": u8, "seed": np.array(SEED), "image_seed": np.array(IMAGE_SEED)}
    for z in Z_DIMS:
        sd = synth.vaegan_encoder_state_dict(SEED, z)
        e = vg.Encoder(z)
        print("z_dim", z, "keys:", e.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True))
        e.eval()
        with torch.no_grad():
            mu32, lv32 = e.encode(torch.from_numpy(x32))
            e64 = e.double()
            mu64, lv64 = e64.encode(torch.from_numpy(x32).double())
        out["mu32_z%d" % z], out["logvar32_z%d" % z] = mu32.numpy(), lv32.numpy()
        out["mu64_z%d" % z], out["logvar64_z%d" % z] = mu64.numpy(), lv64.numpy()
        print("  mu std %.3f logvar std %.3f; float32 vs float64: %.2e / %.2e" % (mu64.std(), lv64.std(), np.abs(mu32.numpy() - mu64.numpy()).max(),
                                                                                 np.abs(lv32.numpy() - lv64.numpy()).max()))
    np.savez(os.path.join(HERE, "vaegan_enc.npz"), **out)


if __name__ == "__main__":
    main()
