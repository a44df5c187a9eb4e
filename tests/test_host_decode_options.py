"""CPU test of what DiCoWForConditionalGeneration.generate derives once for both of its paths: the ``ctc`` dict and the default
prompt reach the decoder the same way from the single-pass path and from the long-form path.  No GPU needed."""
from types import SimpleNamespace

import torch

from tests.test_host_repetition import _Recorder, _model, generation


class _PromptRecorder(_Recorder):
    """The recorder of test_host_repetition, which also keeps the prompt of every call."""
    def __init__(self):
        super().__init__()
        self.prompts = []

    def generate(self, feats, stno, prompt, n_new, **kw):
        self.prompts.append(prompt)
        return super().generate(feats, stno, prompt, n_new, **kw)

    def beam_search(self, feats, stno, prompt, max_length, num_beams, **kw):
        self.prompts.append(prompt)
        return super().beam_search(feats, stno, prompt, max_length, num_beams, **kw)


def test_single_pass_and_long_form_hand_over_the_same_ctc_dict_and_prompt(monkeypatch):
    model, cfg = _model()
    W = 2 * cfg.max_source_positions
    no_ts = 399

    class Tok:
        prefix_tokens = [501, 3, no_ts]
        upper_cased_tokens = {5: 6, 8: 9}
        pad_token_id = 499

        def get_vocab(self):
            return {"<|0.00|>": no_ts + 1, "Ġ": 7}

    model.tokenizer = Tok()
    gc = SimpleNamespace(eos_token_id=500, pad_token_id=500, no_timestamps_token_id=no_ts, ctc_weight=0.3)
    single, long_form = _PromptRecorder(), _PromptRecorder()
    model._decoder = single
    monkeypatch.setattr(generation, "GreedyDecoder", lambda model, use_graphs=False: long_form)
    for beams in (1, 2):
        model.generate(input_features=torch.zeros(2, 80, W), stno_mask=torch.zeros(2, 4, W // 2), generation_config=gc, max_new_tokens=4,
                       num_beams=beams)
        model.generate(input_features=torch.zeros(2, 80, W + 20), stno_mask=torch.zeros(2, 4, (W + 20) // 2), generation_config=gc,
                       attention_mask=torch.ones(2, W + 20, dtype=torch.long), max_new_tokens=4, num_beams=beams)
    assert [n for n, _ in single.calls] == ["generate", "beam_search"]
    assert [n for n, _ in long_form.calls] == ["generate"] * 2 + ["beam_search"] * 2              # (two windows per call)
    want = dict(weight=0.3, first_timestamp=no_ts + 1, upper_cased=[(5, 6), (8, 9)], prefix_len=3)
    for _, kw in single.calls + long_form.calls:
        assert kw["ctc"] == want
    # the default prompt: start + prefix tokens per row; the long form predicts timestamps, so <|notimestamps|> is left out
    for p in single.prompts:
        assert p.tolist() == [[501, 3, no_ts]] * 2
    for p in long_form.prompts:
        assert p.tolist() == [[t for t in single.prompts[0][0].tolist() if t != no_ts]] * 2
    # without a CTC weight neither path builds the dict
    n = len(single.calls), len(long_form.calls)
    gc.ctc_weight = 0.0
    model.generate(input_features=torch.zeros(2, 80, W), stno_mask=torch.zeros(2, 4, W // 2), generation_config=gc, max_new_tokens=4)
    model.generate(input_features=torch.zeros(2, 80, W + 20), stno_mask=torch.zeros(2, 4, (W + 20) // 2), generation_config=gc,
                   attention_mask=torch.ones(2, W + 20, dtype=torch.long), max_new_tokens=4)
    assert all(kw["ctc"] is None for _, kw in single.calls[n[0]:] + long_form.calls[n[1]:])
