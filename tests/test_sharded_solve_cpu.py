"""Host-only pins of the sharded block solve (aniso_block_solve_sharded_dev, DESIGN.md
§3.17): the symbol and its place in the public header, the Python wrapper's argument
checks, and the refusal that needs no device."""
import ctypes
import gc
import os
import re

import numpy as np
import pytest

import aniso_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "aniso_block_solve_sharded_dev"


def test_symbol_is_exported_and_public():
    assert NAME in aniso_amd.exported_symbols()
    assert NAME in aniso_amd.exported_symbols(public_only=True)
    lib = aniso_amd.lib()
    assert hasattr(lib, NAME)
    assert len(getattr(lib, NAME).argtypes) == 13
    assert callable(aniso_amd.Aniso.block_solve_sharded_dev)
    from aniso_amd import dist

    assert callable(dist.native_block_solve)


def test_header_states_the_contract():
    with open(os.path.join(ROOT, "include", "aniso_mi355x.h")) as f:
        text = f.read()
    at = text.index(f"int {NAME}(")
    doc = re.sub(r"\s*\*?\s+", " ", text[text.rfind("/*", 0, at):at])
    for phrase in ("(restart + 1) x ks x owned", "(ks, N) input buffer", "aniso_block_op_sharded_dev",
                   "SAME BITS", "another rank refused", "tree order".upper()):
        assert phrase in doc, phrase


def test_wrapper_rejects_wrong_shapes_and_dtypes():
    torch = pytest.importorskip("torch")
    ks = 3
    h = aniso_amd.Aniso(8, 1, ks, 0.8, 10, 4, 20)
    h.set_shard(0, 2)
    own = h.n_owned()
    good = torch.zeros(ks, own, dtype=torch.float64)  # right shape, but not a CUDA tensor
    bad = [
        (good, good.clone()),                                                  # host memory
        (torch.zeros(ks, own, dtype=torch.float32), good),                     # dtype
        (torch.zeros(ks - 1, own, dtype=torch.float64), good),                 # rows
        (torch.zeros(ks, own - 1, dtype=torch.float64), good),                 # fewer than owned columns
        (torch.zeros(ks * own, dtype=torch.float64), good),                    # not 2-d
        (np.zeros((ks, own)), good),                                           # not a tensor
    ]
    for rhs, x in bad:
        with pytest.raises(aniso_amd.AnisoError) as e:
            h.block_solve_sharded_dev(rhs, x, restart=5, maxit=1)
        assert e.value.code == 1, str(e.value)


def test_sharded_handle_before_set_coeff_is_a_state_error_without_a_device():
    """No communicator, no coefficients: ANISO_ERR_STATE (the error of
    aniso_block_op_sharded_dev there) before any device call -- the dummy pointers are
    never read."""
    # a handle of an earlier test that is garbage in a reference cycle is destroyed when the
    # collector next runs, and aniso_destroy, like every call, resets this thread's last
    # error: collect now, so that none can fall between a call below and its aniso_last_error
    gc.collect()
    ks = 3
    h = aniso_amd.Aniso(8, 1, ks, 0.8, 10, 4, 20)
    h.set_shard(1, 2)
    own = h.n_owned()
    dummy = np.zeros(ks * own)
    it, rr = ctypes.c_int(7), ctypes.c_double(7.0)
    lib = aniso_amd.lib()
    code = lib.aniso_block_solve_sharded_dev(h.address, dummy.ctypes.data, own, dummy.ctypes.data, own, 5, 1e-11, 1,
                                             None, 0, ctypes.byref(it), ctypes.byref(rr), None)
    assert code == 3, code
    buf = ctypes.create_string_buffer(1024)
    lib.aniso_last_error(buf, len(buf))
    solve_msg = buf.value.decode()
    code_op = lib.aniso_block_op_sharded_dev(h.address, 2, dummy.ctypes.data, h.N, dummy.ctypes.data, h.N, None)
    lib.aniso_last_error(buf, len(buf))
    assert (code_op, buf.value.decode()) == (code, solve_msg)
    assert it.value == 7 and rr.value == 7.0 and not dummy.any()
