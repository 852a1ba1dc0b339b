"""What the stream shares with the session pool since it runs on the pool's engine (csrc/ls_chain_api.cpp: session_open, session_push):
the speaker style that a round of the same slots finds in place, the rings fed by one strided copy per run of slots fed alike
(feed_copies, csrc/ls_chain_plan.cpp), and the captured loops a session opened on unmoved buffers keeps.  TED, ddim, 12 executed steps per
window; the speakers and the loop of public calls are tests/test_gpu_long_pool.py's."""
import pytest
import torch

from livelyspeaker_amd import long_form
from test_gpu_long_pool import SPEAKERS, _join, _oracle, _speakers
from test_gpu_long_stream import DEV, S, STRIDE, T, _parts

pytestmark = pytest.mark.gpu


def _feed(pool, y, who, fed, lengths):
    """One push of ``lengths[s]`` further samples of the speaker in slot s: {speaker: its new frames}."""
    audio = torch.zeros(len(lengths), max(lengths), device=DEV)
    for s, n in enumerate(lengths):
        if n:
            audio[s, :n] = y["audio"][SPEAKERS[who[s]], fed[who[s]]:fed[who[s]] + n]
            fed[who[s]] += n
    frames, counts = pool.push(audio, lengths)
    return {who[s]: frames[s, :, :, :int(c)] for s, c in enumerate(counts) if c}


def test_a_round_of_the_same_slots_is_styled_again_after_a_join():
    """Slots [0, 1] run a round as speakers A and B; B leaves and C -- another speaker id, another scale -- joins slot 1; the next round
    holds slots [0, 1] again.  Speaker style kept from the first round would give C the style of B."""
    parts, y = _parts("ted", "ddim"), _speakers("ted")
    cfg, model, diffusion, sampler, skip, _ = parts
    AL = cfg.audio_len
    assert int(y["vid_indices"][1]) != int(y["vid_indices"][2]) and float(y["scale"][1]) != float(y["scale"][2])
    log = ((("A", 0, AL), ("B", 0, AL)), (("A", 1, AL + STRIDE), ("C", 0, AL)))
    want, batches = _oracle("ted", "ddim", 89, log)
    assert batches == [2, 2]
    torch.manual_seed(89)
    pool = long_form.open_pool(diffusion, model, 2, sampler=sampler, skip_timesteps=skip)
    who, fed = {}, {k: 0 for k in SPEAKERS}
    who[_join(pool, y, "A")], who[_join(pool, y, "B")] = "A", "B"
    first = _feed(pool, y, who, fed, [AL, AL])
    assert pool.leave(1).shape[2] == 0                      # B ends on a window's last sample: nothing is owed
    who[_join(pool, y, "C")] = "C"
    assert who == {0: "A", 1: "C"}
    second = _feed(pool, y, who, fed, [STRIDE, AL])
    tail, counts = pool.close()
    assert counts.tolist() == [0, 0] and pool.slots["windows_run"].tolist() == [2, 1]
    got = {"A": torch.cat([first["A"], second["A"]], dim=2), "B": first["B"], "C": second["C"]}
    assert [int(got[k].shape[2]) for k in "ABC"] == [T + S, T, T]
    for k in "ABC":
        print(f"speaker {k}: max |pool - public loops| = {float((got[k] - want[k]).abs().max()):.3e}")
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))


def test_slots_fed_alike_share_a_copy_and_the_slot_beside_them_has_its_own():
    """Capacity 3: slots 0 and 1 are fed alike -- one run, one strided copy -- and slot 2 stays one sample behind -- a run of its own.
    The third push passes the ring's end (audio_len + 2 * 32000 samples into a ring of audio_len + 32000), after one sample for the
    pair and after two for slot 2.  Under Philox every round draws at the pool's key, and so does the loop of public calls."""
    parts, y = _parts("ted", "ddim"), _speakers("ted")
    cfg, model, diffusion, sampler, skip, _ = parts
    AL = cfg.audio_len
    ring = (AL + STRIDE + 3) // 4 * 4
    assert AL + STRIDE <= ring < AL + 2 * STRIDE            # the third push wraps, the second does not
    log = ((("A", 0, AL), ("B", 0, AL)),
           (("A", 1, AL + STRIDE), ("B", 1, AL + STRIDE), ("C", 0, AL - 1 + STRIDE)),
           (("A", 2, AL + 2 * STRIDE), ("B", 2, AL + 2 * STRIDE), ("C", 1, AL - 1 + 2 * STRIDE)),
           (("C", 2, AL - 1 + 2 * STRIDE),))                # the close: C's last window, one sample short, zero-padded
    diffusion.noise_source, diffusion.philox_seed = "philox", 0x0DD5_1DE5
    try:
        want, batches = _oracle("ted", "ddim", 97, log)
        assert batches == [2, 3, 3, 1]
        pool = long_form.open_pool(diffusion, model, 3, sampler=sampler, skip_timesteps=skip)
        who, fed = {}, {k: 0 for k in SPEAKERS}
        for k in "ABC":
            who[_join(pool, y, k)] = k
        parts_of = {k: [] for k in "ABC"}
        for lengths in ([AL, AL, AL - 1], [STRIDE] * 3, [STRIDE] * 3):
            for k, f in _feed(pool, y, who, fed, lengths).items():
                parts_of[k].append(f)
        tail, counts = pool.close()
        assert counts.tolist() == [0, 0, S] and pool.slots["windows_run"].tolist() == [3, 3, 3]
        parts_of["C"].append(tail[2, :, :, :S])
    finally:
        diffusion.noise_source, diffusion.philox_seed, diffusion.sample_offset = "torch_cpu", None, 0
    for k in "ABC":
        got = torch.cat(parts_of[k], dim=2)
        assert got.shape[2] == T + 2 * S
        print(f"speaker {k}: max |pool - public loops| = {float((got - want[k]).abs().max()):.3e}")
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want[k]), (k, float((got - want[k]).abs().max()))


def test_a_stream_opened_again_at_the_same_batch_replays_the_captured_loop():
    """No buffer a captured loop holds by address moves between two streams at one batch on one engine, so the second stream's first
    window is a replay of the loop the first one captured."""
    parts = _parts("ted", "ddim")
    cfg, model, diffusion, sampler, skip, y = parts
    first = y["audio"][:, :cfg.audio_len].contiguous()
    outs, replays = [], []
    for rep in range(2):
        st = long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], sampler=sampler, skip_timesteps=skip)
        torch.manual_seed(101)
        outs.append(st.push(first))
        t = model.model.engine().timing()
        assert outs[-1].shape[3] == T and t["n_segments"] == 1
        replays.append(t["graph_replayed"])
        assert st.close().shape[3] == 0
    assert torch.equal(outs[0], outs[1])
    if diffusion.use_graph:
        assert replays[1] == 1, replays
