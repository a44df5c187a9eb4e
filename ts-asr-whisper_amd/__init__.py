"""MI355X-native (gfx950) DiCoW / SE-DiCoW training-step hot path.

Host side (Python, mirrors the reference's module surface: ``FDDT``, ``DiCoWEncoder``,
``DiCoWForConditionalGeneration``, ``DiCoWConfig``) over the C-ABI library ``libdicow_hip.so``
(hand-written HIP kernels, see ``csrc/`` and ``include/dicow_hip.h``).

There is NO CPU fallback: every op raises if the HIP library is missing or the tensors are not
on a GPU.  The CPU oracle lives in ``oracle/`` and is test infrastructure only.
"""
from . import _lib  # noqa: F401
from .config import DiCoWConfig, PRESETS  # noqa: F401
from .modeling import (FDDT, DiCoWEncoder, DiCoW, DiCoWForConditionalGeneration, SpeakerCommunicationBlock,  # noqa: F401
                       shift_tokens_right, build_ts_tables, LoRALinear, add_decoder_lora, merge_lora, save_adapter, load_adapter,
                       freeze_for_ctc_pretraining)
from .ctc_decoding import ctc_greedy_decode, chunked_ctc_logits  # noqa: F401
from .generation import phrase_sequences, sample_tokens, sampling_options  # noqa: F401
from .ctc_align import (CtcAlignment, ctc_forced_align, token_timestamps, word_timestamps, align_segments,  # noqa: F401
                        words_as_segments)
from .wave_augment import NoiseBank, plan_background_noise, mix_background_noise, WaveFrontEnd  # noqa: F401
from .diar_front_end import (SpeakerSegments, stno_masks, select_enrollment_windows, draw_enrollment_window,  # noqa: F401
                             MeetingFrontEnd)
from .enrollment_mix import (EnrollmentBank, plan_enrollment_mixtures, mix_enrollments, enrollment_stno,  # noqa: F401
                             EnrollmentMixFrontEnd)
from .wave_intake import (ResamplePlan, resample_plan, resample_segments, resample, read_wav, load_recording)  # noqa: F401
from .scoring import (edit_counts, Vocabulary, word_error_counts, error_measures, make_compute_metrics, cp_wer, tcp_wer,  # noqa: F401
                      pseudo_word_intervals, hungarian, orc_counts, orc_wer, tcorc_wer, filter_empty_segments, create_vad_mask,
                      find_group_splits, map_utterance_to_split, merge_streams, create_dummy_seg_list, session_tcorc_wer,
                      session_orc_wer, session_metrics, aggregate_session_metrics, edit_alignments, alignment_chunks, alignment_rows,
                      word_alignments, format_alignment, session_alignment, error_breakdown, save_alignment_report)
from .diar_scoring import (unscored_intervals, diar_score_counts, split_counts, mapping_from_counts, error_from_counts,  # noqa: F401
                           jaccard_from_counts, aggregate_diarization_scores, diarization_error, jaccard_error, optimal_mapping,
                           score_diarizations)
from .hyp_cleanup import (repeating_ngram_cuts, truncate_repeating_ngrams, truncate_at_repeating_ngram,  # noqa: F401
                          session_hypotheses)
from .significance import (bootstrap_sums, percentile_interval, ratio_interval, compare_ratios, session_metric_intervals,  # noqa: F401
                           compare_session_metrics, wer_interval, compare_wer)
from .optim import DiCoWAdamW, clip_grad_norm_, dicow_optimizer  # noqa: F401
from .watch import tensor_stats, TensorStats, GradWatch, WatchCallback, as_wandb, jsonl_sink  # noqa: F401

__all__ = ["DiCoWConfig", "FDDT", "DiCoWEncoder", "DiCoW", "DiCoWForConditionalGeneration", "SpeakerCommunicationBlock",
           "LoRALinear", "add_decoder_lora", "merge_lora", "save_adapter", "load_adapter", "DiCoWAdamW", "clip_grad_norm_", "dicow_optimizer",
           "ctc_greedy_decode", "chunked_ctc_logits", "freeze_for_ctc_pretraining", "NoiseBank", "plan_background_noise", "mix_background_noise",
           "WaveFrontEnd", "SpeakerSegments", "stno_masks", "select_enrollment_windows", "draw_enrollment_window", "MeetingFrontEnd",
           "EnrollmentBank", "plan_enrollment_mixtures", "mix_enrollments", "enrollment_stno", "EnrollmentMixFrontEnd",
           "ResamplePlan", "resample_plan", "resample_segments", "resample", "read_wav", "load_recording",
           "edit_counts", "Vocabulary", "word_error_counts", "error_measures", "make_compute_metrics", "cp_wer", "tcp_wer",
           "pseudo_word_intervals", "hungarian", "orc_counts", "orc_wer", "tcorc_wer", "filter_empty_segments", "create_vad_mask",
           "find_group_splits", "map_utterance_to_split", "merge_streams", "create_dummy_seg_list", "session_tcorc_wer", "session_orc_wer",
           "session_metrics", "aggregate_session_metrics", "edit_alignments", "alignment_chunks", "alignment_rows", "word_alignments",
           "format_alignment", "session_alignment", "error_breakdown", "save_alignment_report", "unscored_intervals", "diar_score_counts", "split_counts", "mapping_from_counts",
           "error_from_counts", "jaccard_from_counts", "aggregate_diarization_scores", "diarization_error", "jaccard_error", "optimal_mapping",
           "score_diarizations", "CtcAlignment", "ctc_forced_align", "token_timestamps", "word_timestamps", "align_segments",
           "words_as_segments", "tensor_stats", "TensorStats", "GradWatch", "WatchCallback", "as_wandb", "jsonl_sink", "repeating_ngram_cuts", "truncate_repeating_ngrams", "truncate_at_repeating_ngram", "session_hypotheses",
           "bootstrap_sums", "percentile_interval", "ratio_interval", "compare_ratios", "session_metric_intervals", "compare_session_metrics",
           "wer_interval", "compare_wer", "phrase_sequences", "sample_tokens", "sampling_options"]
