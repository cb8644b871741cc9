"""GPU: uhc_env_create refuses a descriptor by name before it touches the device (the plan: tests/test_env_plan_cpu.py has every refusal), and a refused call
leaves the batch as it was: the same batch then carries a valid env through a reset and a step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_refusals_raise_their_text_and_the_batch_still_makes_an_env(model, ctrl):
    import torch
    from tests.test_gpu_env import REWARD_W, _expert
    from uhc_amd import sim as S
    from uhc_amd._capi import env_desc
    from uhc_amd._lib import UhcError
    n = 2
    sb = S.SimBatch(model, ctrl, n)
    for fields, text in ((dict(obs_v=7), "uhc_env_create: obs_v must be 0 .. 6"),
                         (dict(obs_v=3, fut_frames=65), "uhc_env_create: obs_v 3 needs 1 <= fut_frames <= 64, skip >= 0"),
                         (dict(num_obj=1), "uhc_env_create: num_obj exceeds the free bodies at the end of the model")):
        with pytest.raises(UhcError) as ei:
            S.EnvBatch(sb, env_desc(model, **fields))
        assert text in str(ei.value)
    eb = S.EnvBatch(sb, env_desc(model, obs_v=2, has_shape=True, reward_weights=REWARD_W))
    assert eb.obs_dim == 657
    expert = _expert()
    eb.set_bank(torch.from_numpy(S.pack_expert_frames(expert)), torch.tensor([0], dtype=torch.int32), torch.from_numpy(np.r_[np.zeros(16), 2.0][None]))
    ids = torch.arange(n, dtype=torch.int32)
    eb.assign(ids, torch.zeros(n, dtype=torch.int32), torch.tensor([0, 5], dtype=torch.int32), torch.tensor([30, 20], dtype=torch.int32))
    eb.reset(ids.cuda(), None)
    sb.sync()
    assert np.isfinite(eb.field(S.E_OBS).cpu().numpy()).all()
    eb.step(torch.zeros(n, ctrl.action_dim, dtype=torch.float64).cuda(), None)
    sb.sync()
    obs = eb.field(S.E_OBS).cpu().numpy()
    assert obs.shape[-1] * n == obs.size == 2 * 657 and np.isfinite(obs).all()
    assert (eb.field(S.E_CUR_T).cpu().numpy() == 1).all()
