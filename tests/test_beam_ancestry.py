"""CPU test of the beam search's ancestry table (generation.advance_ancestry): caches that are never reordered, read through the
table, hold exactly what physically reordered caches hold."""
import torch

import amd_pkg

amd_pkg.load()


def test_ancestry_table_equals_physical_reorder():
    """Model A: a toy cache [R, Lmax] with a unique tag per (slot, position), reordered by index_select after every step exactly
    as beam_search(reorder_caches=True) does.  Model B: the same writes, never reordered, read through the table.  After every
    step cacheB[anc[r, t], t] == cacheA[r, t] for all rows and all written positions, and the unwritten columns of the table
    still point at the row's own slot (the next step reads its own key there)."""
    from ts_asr_whisper_amd.generation import advance_ancestry
    B0, K, steps, Lmax = 2, 5, 30, 40
    R = B0 * K
    g = torch.Generator().manual_seed(1234)
    cache_a = torch.full((R, Lmax), -1, dtype=torch.long)
    cache_b = cache_a.clone()
    anc = torch.arange(R, dtype=torch.int32)[:, None].repeat(1, Lmax)
    rows, cols = torch.arange(R), torch.arange(Lmax)
    for pos in range(steps):
        cur = pos + 1
        tag = rows * 1000 + pos                                       # every row writes position `pos` into its own slot
        cache_a[:, pos] = tag
        cache_b[:, pos] = tag
        beam_idx = (torch.randint(0, K, (B0, K), generator=g) + (torch.arange(B0) * K)[:, None]).reshape(-1)
        cache_a[:, :cur] = cache_a[:, :cur].index_select(0, beam_idx)
        out = advance_ancestry(anc, beam_idx, pos)
        assert out is anc and anc.dtype == torch.int32                # in place on the persistent buffer
        through = cache_b[anc[:, :cur].long(), cols[None, :cur]]
        assert torch.equal(through, cache_a[:, :cur]), pos
        assert torch.equal(anc[:, cur:], rows.to(torch.int32)[:, None].expand(R, Lmax - cur)), pos
        assert bool(((anc[:, :cur].long() // K) == (rows // K)[:, None]).all())        # a row never leaves its window's slots
    assert len(set(cache_a[:, :steps].reshape(-1).tolist())) > R      # (the draw really mixed the beams)
