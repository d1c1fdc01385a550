"""GPU: the project's own PGGAN at steps=7 makes 512 x 512 banks (3 x 512 x 512 = 786432 values per image, beyond the int32-norm limit of
262143); the exact L2 search takes them on the wide path, generated chunk by chunk or materialised, and equals the C oracle on the same
bytes."""
import numpy as np
import pytest

import gpu_common  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gl():
    import ganleaks_amd
    return ganleaks_amd


def test_generated_512_bank_l2_matches_oracle(gl, synth):
    import c_oracle
    from ganleaks_amd.attack import GeneratedBank
    from ganleaks_amd.gan_models.pggan.model_torch import Generator
    gen = Generator(64, 512, 3)
    gen.load_state_dict(synth.pggan_state_dict(4321 + 512, 64, 512))
    z = synth.latent(41, 72, 64)
    bank = gen.generate_u8(z, steps=7, alpha=1.0)
    hb = bank.numpy()
    assert hb.shape == (72, 3, 512, 512) and hb.dtype == np.uint8
    d = 3 * 512 * 512
    planted = [7, 50, 63]
    # perturbed members, an exact member, a member in the truncated tail (72 -> 64 rows) and fresh images
    q = np.concatenate([synth.perturb_u8(5, hb[planted], 4.0), hb[[20]], synth.perturb_u8(6, hb[[70]], 4.0),
                        synth.lowpass_u8_images(8, 2, 512)])
    od, oi, _ = c_oracle.knn_l2_u8(hb, q, 16)
    dr, ir = gl.attack(q, bank, distance="l2", batch_size=16)
    assert np.array_equal(ir, oi) and np.array_equal(dr, od)
    assert ir[:4].tolist() == planted + [20] and dr[3] == 0 and ir[4] < 64
    ds, is_ = gl.attack(q, GeneratedBank(gen, z, steps=7, alpha=1.0), distance="l2", batch_size=16, chunk_bytes=10 * 2 * d)
    assert np.array_equal(is_, oi) and np.array_equal(ds, od)
