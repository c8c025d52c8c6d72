"""The hypothesis bookkeeping of beam search on the host: HF 4.31's BeamSearchScorer / BeamHypotheses for one sample and one returned
sequence, replayed over the candidates the device recorded (ops.beam_topk).  Hypotheses never influence which beams continue — that is the
device's selection — they only decide when the search stops and which answer wins, so the host can run this after the fact, at every look
of the captured decode loop.  Pure Python on Python floats, as HF's scorer works on `.item()`s; no torch in here."""


class BeamScorer:
    """Feed step(candidates) once per decode step, in order, until it returns True (done) or max_new_tokens steps are in; then finalize().

    candidates: the step's 2 * num_beams (score, parent beam, token) in rank order — value descending, flat index ascending.
    Step t (t = 0, 1, ...) ranks the continuations of beams that hold t generated tokens."""

    def __init__(self, num_beams, length_penalty=1.0, early_stopping=False, eos_token_id=2, length_base=0, max_new_tokens=512):
        if early_stopping not in (False, True):
            raise ValueError(f"BeamScorer: early_stopping={early_stopping!r} (only False and True are built)")
        self.num_beams, self.length_penalty, self.early_stopping = int(num_beams), float(length_penalty), bool(early_stopping)
        self.eos_token_id, self.length_base, self.max_new_tokens = int(eos_token_id), int(length_base), int(max_new_tokens)
        self.beams = [[] for _ in range(self.num_beams)]        # generated tokens of the running beams
        self.scores = [0.0] * self.num_beams                    # their summed log-probabilities
        self.hyps = []                                          # (score, tokens) in the order they were added
        self.worst_score = 1e9
        self.done = False
        self.steps = 0

    def length(self, n_generated):
        """THE length convention, in this one expression: a sequence's length is length_base + its generated tokens, with length_base = the
        prompt row's id count — to our knowledge HF 4.31's rule (hyp.shape[-1] and cur_len both count the prompt; later releases count the
        generated tokens only).  Unverified against the 4.31 source; it only matters for length_penalty != 0."""
        return self.length_base + n_generated

    def _add(self, tokens, sum_logprobs):
        """BeamHypotheses.add: keep the num_beams best by sum_logprobs / length ** length_penalty."""
        score = sum_logprobs / (self.length(len(tokens)) ** self.length_penalty)
        if len(self.hyps) < self.num_beams or score > self.worst_score:
            self.hyps.append((score, list(tokens)))
            if len(self.hyps) > self.num_beams:
                worst = min(range(len(self.hyps)), key=lambda i: self.hyps[i][0])       # (the first of equal worst, as HF's sorted()[0])
                del self.hyps[worst]
                self.worst_score = min(s for s, _ in self.hyps)
            else:
                self.worst_score = min(score, self.worst_score)

    def _is_done(self, best_sum_logprobs, n_generated):
        """BeamHypotheses.is_done at a step whose beams hold n_generated tokens."""
        if len(self.hyps) < self.num_beams:
            return False
        if self.early_stopping:
            return True
        return self.worst_score >= best_sum_logprobs / self.length(n_generated) ** self.length_penalty

    def step(self, candidates):
        """BeamSearchScorer.process for one step -> done.  The running beams advance by the first num_beams non-eos candidates (the
        device's selection); an eos candidate of rank < num_beams ends its parent beam as a hypothesis, one of a lower rank is ignored."""
        assert not self.done and self.steps < self.max_new_tokens and len(candidates) == 2 * self.num_beams
        t, nb = self.steps, self.num_beams
        nxt_beams, nxt_scores = [], []
        for rank, (score, parent, token) in enumerate(candidates):
            score, parent, token = float(score), int(parent), int(token)
            if token == self.eos_token_id:
                if rank < nb:
                    self._add(self.beams[parent], score)
            elif len(nxt_beams) < nb:
                nxt_beams.append(self.beams[parent] + [token])
                nxt_scores.append(score)
        assert len(nxt_beams) == nb, "fewer than num_beams continuations among the candidates"
        self.done = self._is_done(max(float(c[0]) for c in candidates), t)
        self.beams, self.scores, self.steps = nxt_beams, nxt_scores, t + 1
        return self.done

    def finalize(self):
        """BeamSearchScorer.finalize -> (generated tokens of the winner, its score).  A search that ran into max_new_tokens adds its running
        beams first; the best hypothesis wins (the latest added among equals); the eos is appended when the answer is shorter than
        max_new_tokens."""
        if not self.done:
            for tokens, score in zip(self.beams, self.scores):
                self._add(tokens, score)
        order = sorted(range(len(self.hyps)), key=lambda i: self.hyps[i][0])
        score, tokens = self.hyps[order[-1]]
        tokens = list(tokens)
        if len(tokens) < self.max_new_tokens:
            tokens.append(self.eos_token_id)
        return tokens, score
