"""`models.t5_segmem_v2_with_prev` — drop-in for the paper's MR-MT3 model
(models/t5_segmem_v2_with_prev.py:38-296): memory from an explicit `targets_prev` tensor in
training, and from the previous segment's generated tokens in `generate`."""
import torch

from mrmt3.module import MT3Module


class T5SegMemV2WithPrev(MT3Module):
    VARIANT = "segmem_v2_with_prev"

    def __init__(self, config, segmem_num_layers: int = 1, segmem_length: int = 64, compute_dtype=None):
        super().__init__(config, segmem_num_layers=segmem_num_layers, segmem_length=segmem_length,
                         compute_dtype=compute_dtype or torch.bfloat16)

    def generate_songs(self, songs, max_length=1024, num_beams=1, length_penalty=1.0, bad_token_ids=None,
                       return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, constrained=False,
                       **kwargs):
        """Several recordings at once, one decode-batch row per recording (each keeps its own memory chain);
        row results equal `generate` on that recording alone.  Not in the reference, which is sequential.
        `num_beams` > 1: one beam group per recording, each equal to `generate_beam` on that recording alone.
        `return_logprobs`: (ids per recording, per-token log-probabilities per recording).
        `do_sample` (with `num_beams=1`): the tokens are drawn (`mrmt3.decode.generate_songs`).
        `constrained`: every recording decodes under the event grammar, each segment starting from the notes the one before
        left sounding."""
        from mrmt3.decode import generate_songs
        return generate_songs(self, songs, max_length=max_length, num_beams=num_beams, length_penalty=length_penalty,
                              bad_token_ids=bad_token_ids, return_logprobs=return_logprobs,
                              do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                              constrained=constrained)
