"""The pass decomposition of the block operator beyond 8 Fourier blocks (DESIGN.md
§3.9.1), host side: the plan, and the sub-mix identity the device passes rest on."""
import numpy as np
import pytest

import aniso_amd


@pytest.mark.parametrize("ks,want", [(1, (1, 1)), (5, (5, 1)), (8, (8, 1)), (9, (8, 2)), (12, (8, 2)), (16, (8, 2)),
                                     (17, (8, 3))])
def test_block_pass_plan(ks, want):
    assert aniso_amd.block_pass_plan(ks) == want


def test_block_pass_plan_rejects_no_blocks():
    with pytest.raises(aniso_amd.AnisoError) as e:
        aniso_amd.block_pass_plan(0)
    assert e.value.code == 1


@pytest.mark.parametrize("chi", [True, False])
@pytest.mark.parametrize("g", [0.8, 0.95])
@pytest.mark.parametrize("ks", [9, 12, 16, 17])
def test_sub_mixes_of_the_passes_tile_the_block_mixes(ks, g, chi):
    """Pass (I, J) takes sub[m][i][b] = mix[m][8 I + i][8 J + b], zero outside ks: put
    back at (8 I, 8 J) the passes' sub-mixes are block_mixes(ks, g, chi) exactly, so the
    sum of the passes is the block operator.  Also the two sets of weights a pass's
    harmonic launch is given: hw_B = mix[B][0][B] (w_0, or 2 w_B) and, for I == J, the
    diagonal weight dw_i = mix[0][i][i] = w_i."""
    mix = aniso_amd.block_mixes(ks, g, chi)
    chunk, P = aniso_amd.block_pass_plan(ks)
    assert chunk == 8 and P == -(-ks // 8)
    nm = 2 * ks - 1
    back = np.zeros_like(mix)
    for I in range(P):
        for J in range(P):
            i0, b0 = chunk * I, chunk * J
            sub = np.zeros((nm, chunk, chunk))
            ni, nb = min(chunk, ks - i0), min(chunk, ks - b0)
            sub[:, :ni, :nb] = mix[:, i0:i0 + ni, b0:b0 + nb]
            assert not sub[:, ni:, :].any() and not sub[:, :, nb:].any()  # padded rows / inputs carry no weight
            back[:, i0:i0 + ni, b0:b0 + nb] += sub[:, :ni, :nb]
    assert np.array_equal(back, mix)
    w = np.array([(g ** b - g ** ks) / (1 - g ** ks) if chi else 1.0 for b in range(ks)])
    hw = np.array([mix[B, 0, B] for B in range(ks)])
    assert np.allclose(hw, np.where(np.arange(ks) == 0, w, 2 * w), rtol=1e-15, atol=0)
    assert np.allclose([mix[0, i, i] for i in range(ks)], w, rtol=1e-15, atol=0)
