"""CPU-only checks around the device backend of the linear-assignment instance loss (ABI 27): the shared case generators meet the
conditions the GPU tests rely on, the backend switches validate their values, and the new ABI entries are declared, exported and bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import lsap_cases

NEW_SYMBOLS = ("clift_lsap", "clift_assign_work_bytes", "clift_assign_loss")


def test_matching_cases_have_a_margin_above_the_fp32_noise():
    """(a) every image of matching_cases(): 31 of them, and the optimum of the oracle's cost matrix is further from the runner-up than twice L
    times 2^-22 -- the device's cost matrix may differ from the oracle's by fp32 round-off without changing the matching."""
    cases = lsap_cases.matching_cases()
    assert len(cases) == 31
    worst = np.inf
    for name, y, f in cases:
        ids, cost = lsap_cases.oracle_cost(y, f)
        L = len(ids)
        assert L == min(len(set(y.tolist())), f.shape[1]) and cost.shape == (L, f.shape[1])
        m, need = lsap_cases.margin(cost), 2 * L * 2.0 ** -22
        worst = min(worst, m / need)
        assert m > need, (name, m, need)
    print(f"smallest margin / (2 L 2^-22): {worst:.2f}")


def test_random_solver_cases_have_a_unique_optimum():
    """(a) the random matrices of solver_cases() have a positive margin: scipy's assignment is THE optimum, and the device solver must return it."""
    kinds = [k for _, k, _ in lsap_cases.solver_cases()]
    assert kinds.count("random") == 9 and kinds.count("integer") == 5 and kinds.count("product") == 2 and kinds.count("nan") == 1
    for name, kind, cost in lsap_cases.solver_cases():
        assert cost.dtype == np.float32 and cost.shape[0] <= cost.shape[1] <= 512
        if kind == "random":
            assert lsap_cases.margin(cost) > 0, name


def test_unknown_backend_is_a_value_error():
    """(b) all three functions refuse a backend they do not know before they look at anything else."""
    from contrastive_lift_amd import loss
    y, f, conf = torch.tensor([1, 2, 1]), torch.zeros(3, 4), torch.ones(3)
    with pytest.raises(ValueError, match="bogus"):
        loss.linear_assignment_loss(f, y, conf, backend="bogus")
    with pytest.raises(ValueError, match="bogus"):
        loss.linear_assignment_loss(f, y, conf, return_grad=True, backend="bogus")
    with pytest.raises(ValueError, match="bogus"):
        loss.create_virtual_gt_with_linear_assignment(y, f, backend="bogus")
    from contrastive_lift_amd.trainer import HotPathTrainer, default_config
    with pytest.raises(ValueError, match="bogus"):
        HotPathTrainer(None, None, default_config(assignment_backend="bogus"))


def test_device_backend_without_a_gpu_tensor_raises_clift_error():
    """No silent fallback: the device backend on host tensors is an error, not the host path."""
    from contrastive_lift_amd import CliftError, loss
    y, f, conf = torch.tensor([1, 2, 1]), torch.zeros(3, 4), torch.ones(3)
    with pytest.raises(CliftError):
        loss.linear_assignment_loss(f, y, conf, return_grad=True, backend="device")
    with pytest.raises(CliftError):
        loss.create_virtual_gt_with_linear_assignment(y, f, backend="device")
    with pytest.raises(CliftError):
        loss.linear_sum_assignment_device(torch.zeros(2, 3))


def _trainer_init_with(cfg):
    """HotPathTrainer.__init__ up to the backend check, on stand-ins: the check needs no model."""
    from contrastive_lift_amd import trainer as tr

    class Arena:
        groups = {}

    class Model:
        num_semantic_classes = 3
        param_flat = torch.zeros(4)
        arena = Arena()

    t = tr.HotPathTrainer.__new__(tr.HotPathTrainer)
    t.setup_optimizers = lambda *a, **k: None
    t.on_train_epoch_start = lambda *a, **k: None
    tr.HotPathTrainer.__init__(t, Model(), None, cfg)
    return t


def test_trainer_config_key():
    """(c) the extension key defaults to the host path, reaches the trainer, and an unknown value is refused at construction."""
    from contrastive_lift_amd.trainer import default_config
    assert default_config().assignment_backend == "host"
    assert _trainer_init_with(default_config()).assignment_backend == "host"
    assert _trainer_init_with(default_config(assignment_backend="device")).assignment_backend == "device"
    with pytest.raises(ValueError, match="assignment_backend"):
        _trainer_init_with(default_config(assignment_backend="gpu"))


def test_command_line_override_reaches_the_config():
    """The train CLI hands Hydra-style overrides to load_config: ``assignment_backend=device`` lands in the tree the trainer reads, and no YAML
    under config/ carries the key (the loaded trees stay key-for-key the reference's)."""
    from contrastive_lift_amd.config import load_config
    cfg_dir = os.path.join(REPO, "config")
    assert getattr(load_config(cfg_dir), "assignment_backend", "host") == "host"
    assert "assignment_backend" not in load_config(cfg_dir)
    for ov in ("assignment_backend=device", "+assignment_backend=device", "template.assignment_backend=device"):
        assert load_config(cfg_dir, overrides=[ov]).assignment_backend == "device"


def test_abi_27_declares_exports_and_binds_the_new_entries():
    """(d) the checks of test_abi.py on the new names: declared in include/clift.h, exported by libclift.so, rows in the ctypes table, and the
    three version numbers at 27."""
    from contrastive_lift_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "clift.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(clift_[a-z0-9_]+)\s*\(", src))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/clift.h"
        assert hasattr(lib, s), f"{s} is not exported by libclift.so"
        assert s in _lib.exported_symbols(), f"{s} has no row in the ctypes table"
    assert sorted(_lib.exported_symbols()) == sorted(declared)
    assert _lib.ABI_VERSION == 27 and _lib.load().clift_version() == 27
    assert _lib.load().clift_assign_work_bytes(1024, 25) >= 16 * 1024 + 4 * 25 * 25
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert re.search(r"ABI 27|\(27;", open(os.path.join(REPO, doc)).read()), doc


def test_host_entry_checks_need_no_gpu():
    """clift_lsap refuses bad sizes before it touches the device: the error strings name the limit."""
    from contrastive_lift_amd import _lib
    lib = _lib.load()
    for args, word in (((None, 4, 0, 1, 5, 4, None, None, None), "L = 5"), ((None, 513, 0, 1, 2, 513, None, None, None), "512"),
                       ((None, 3, 0, 1, 2, 4, None, None, None), "ld = 3"), ((None, 4, 0, -1, 2, 4, None, None, None), "negative"),
                       ((None, 4, 0, 1, 2, 4, None, None, None), "NULL")):
        assert lib.clift_lsap(*args) != 0
        assert word in lib.clift_last_error().decode(), (args, lib.clift_last_error())
    assert lib.clift_lsap(None, 4, 0, 0, 2, 4, None, None, None) == 0           # nb == 0: nothing to do
    assert lib.clift_lsap(None, 4, 0, 3, 0, 4, None, None, None) == 0           # L == 0
