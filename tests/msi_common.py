"""TEST INFRASTRUCTURE shared by tests/test_cpu_msi.py and tests/test_gpu_msi.py: the draws D' under which the un-hoisted
multi-step loop computes what `reuse_encoder=True` computes, and seeded multi-step draws.  Never imported by the product."""
import numpy as np
import torch

PER_CALL = 8  # order shuffles of one conditional backbone call: [c_ser, n_ser, c1, n1, n2, c2, n3, n4]
N_POSITIONS = (1, 3, 4, 6, 7)  # the n-branch's positions among them


def d_prime(draws):
    """D' of draws D: every backbone call k >= 1 repeats the first call's n-branch shuffles,
    perms[8k + j] = perms[j] for j in N_POSITIONS."""
    perms = [np.array(p).copy() for p in draws["perms"]]
    assert len(perms) % PER_CALL == 0
    for k in range(1, len(perms) // PER_CALL):
        for j in N_POSITIONS:
            perms[PER_CALL * k + j] = perms[j].copy()
    return dict(draws, perms=perms)


def seeded_draws(seed, rows, channels, calls):
    """Noise rows and 8 * calls order shuffles from a generator of their own."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.normal(0, 1, size=(rows, channels), dtype=torch.float32, generator=g)
    perms = [torch.randperm(4, generator=g).numpy() for _ in range(PER_CALL * calls)]
    return dict(noise=noise, perms=perms)


def differs_somewhere(draws):
    """D and D' are different draws: some later call's n-branch shuffle is not the first call's."""
    dp = d_prime(draws)
    return any(not np.array_equal(a, b) for a, b in zip(draws["perms"], dp["perms"]))
