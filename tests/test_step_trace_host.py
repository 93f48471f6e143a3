"""The launch sequence of AttackEngine.step_mi / step_l2 for every combination of their options,
pinned on the host (no GPU): ops.call / ops.ptr / ops.stream are replaced by recorders, the
networks by a stub of gradient(), and every launch (kernel name, workspace buffer names, scalar
arguments) is compared with tests/golden/step_trace.json. The wrappers' own host validation still
runs. A launch that is added, dropped, reordered or pointed at another buffer fails the test.

The fixture was recorded from commit 066cdb2, the last one with a method per attack variant
(`python tests/test_step_trace_host.py` rewrites it). Record it again only for a change that is
meant to alter a launch sequence, never to make this test pass."""
import itertools
import json
import os

import pytest
import torch

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "step_trace.json")
N, S = 2, 8
TI = {"none": None, "3taps": (0.25, 0.5, 0.25)}
DI = {"none": None, "apply1": (6, 1, 1, 1), "apply0": (6, 1, 1, 0)}
# VtStep fields: samples, r, seed, image0, step, last
VT = {"none": None, "2samples": (2, 0.125, 12345, 0, 1, False),
      "last": (2, 0.125, 12345, 0, 1, True)}
MU, A, E = 1.0, 2 * 2 / 255, 2 * 8 / 255
UPDATES = ("mia_mi_update", "mia_l2_step", "mia_l2_project")


class _Net:
    """What AttackEngine reads of a network before any launch."""
    size, n_latent = S, 4
    dtype = torch.float32
    device = torch.device("cpu")


def _key(**kw):
    return " ".join(f"{k}={v}" for k, v in kw.items())


def mi_cases():
    for ti, di, nes, si, vt in itertools.product(TI, DI, (False, True), (1, 3), VT):
        yield _key(step="mi", ti=ti, di=di, nesterov=int(nes), si=si, vt=vt), (ti, di, nes, si, vt)


def l2_cases():
    for ti, di, si in itertools.product(TI, DI, (1, 3)):
        yield _key(step="l2", ti=ti, di=di, si=si), (ti, di, si)


class _Recorder:
    """One engine on CPU tensors whose launches are appended to ``trace`` instead of run."""

    def __init__(self, mp):
        from gfa_amd import ops, pgd
        self.trace = []
        self.eng = eng = pgd.AttackEngine(_Net(), _Net(), _Net())
        ws = eng.ws
        eng.N = N
        eng.x0 = torch.zeros(N, 3, S, S)
        eng.nonfinite = ws.get("nonfinite", (N,), torch.int32)
        self.x = ws.get("adv", (N, 3, S, S), torch.float32)
        self.m = ws.get("mi.m", (N, 3, S, S), torch.float32)
        self.named = {"x0": eng.x0}
        mp.setattr(ops, "ptr", self.name)
        mp.setattr(ops, "stream", lambda: "stream")
        mp.setattr(ops, "call", lambda kernel, *args: self.trace.append([kernel, *args]))
        mp.setattr(eng, "gradient", self.gradient)
        copy_ = torch.Tensor.copy_

        def traced_copy(dst, src, *a, **kw):
            self.trace.append(["copy_", self.name(dst), self.name(src)])
            return copy_(dst, src, *a, **kw)
        mp.setattr(torch.Tensor, "copy_", traced_copy)

    def name(self, t):
        """The workspace buffer a tensor lives in, by address range (+ its element offset)."""
        if t is None:
            return None
        for name, b in itertools.chain(self.eng.ws._bufs.items(), self.named.items()):
            off = t.data_ptr() - b.data_ptr()
            if 0 <= off < b.numel() * b.element_size():
                k = off // b.element_size()
                return name if k == 0 else f"{name}+{k}"
        raise AssertionError("a launch reads a tensor outside the workspace")

    def gradient(self, x, loss=None):
        assert loss is None
        self.trace.append(["gradient", self.name(x)])
        return None, None

    def taps(self, ti):
        if TI[ti] is None:
            return None
        self.named["taps"] = self.eng.ti_device_taps(TI[ti])
        return self.named["taps"]


def record():
    """{case: [launch, …]} of the whole grid, on the pgd.py that is imported."""
    from gfa_amd import pgd
    a, e = pgd._f32(A), pgd._f32(E)
    out = {}
    for key, (ti, di, nes, si, vt) in mi_cases():
        with pytest.MonkeyPatch.context() as mp:
            r = _Recorder(mp)
            step_vt = None if VT[vt] is None else pgd.VtStep(*VT[vt])
            r.eng.step_mi(r.x, r.m, MU, a, e, r.taps(ti), DI[di], nes, si, step_vt)
        out[key] = r.trace
    for key, (ti, di, si) in l2_cases():
        with pytest.MonkeyPatch.context() as mp:
            r = _Recorder(mp)
            r.eng.step_l2(r.x, a, e, r.taps(ti), DI[di], si)
        out[key] = r.trace
    return out


@pytest.fixture(scope="module")
def traces():
    return record()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def test_grid_is_the_fixtures(traces, golden):
    assert len(traces) == 72 + 12
    assert sorted(traces) == sorted(golden)


@pytest.mark.parametrize("key", [k for k, _ in itertools.chain(mi_cases(), l2_cases())])
def test_launch_sequence_is_the_recorded_one(traces, golden, key):
    got = json.loads(json.dumps(traces[key]))  # tuples → lists, as the fixture went through
    assert got == golden[key], key


def _chain(trace):
    """The launches between the zeroing of norm.sums and the update kernel(s)."""
    assert trace[0][:2] == ["mia_memset", "norm.sums"]
    first = next(i for i, l in enumerate(trace) if l[0] in UPDATES)
    assert all(l[0] in UPDATES for l in trace[first:])
    return trace[1:first]


def test_gradient_passes_per_chain(traces):
    """Exactly si_scales gradient() calls per chain: one chain per step, 1 + samples with the
    neighbours of a variance-tuned step that is not the last."""
    for key, (ti, di, nes, si, vt) in mi_cases():
        chains = 1 if VT[vt] is None or VT[vt][5] else 1 + VT[vt][0]
        assert sum(l[0] == "gradient" for l in traces[key]) == si * chains, key
    for key, (ti, di, si) in l2_cases():
        assert sum(l[0] == "gradient" for l in traces[key]) == si, key


def test_sums_go_to_the_last_kernel_before_the_update(traces):
    for key, trace in traces.items():
        chain = _chain(trace)
        takes = [i for i, l in enumerate(chain)
                 if any(isinstance(a, str) and a.startswith("norm.sums") for a in l[1:])]
        assert takes == [len(chain) - 1], key
        assert chain[-1][0].endswith("_norms"), key
        # and the update reads the buffer that kernel wrote
        g = trace[len(chain) + 1][3]
        assert g in chain[-1][1:] and g.startswith(("g.", "vt.gt")), key


def test_di_row_with_apply_0_is_no_di(traces):
    for key in traces:
        if "di=apply0" in key:
            assert traces[key] == traces[key.replace("di=apply0", "di=none")], key
        if "di=apply1" in key:
            assert traces[key] != traces[key.replace("di=apply1", "di=none")], key


if __name__ == "__main__":
    cases = json.loads(json.dumps(record()))
    with open(FIXTURE, "w") as f:
        f.write('{"cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: [\n  "
                           + ",\n  ".join(json.dumps(l) for l in v) + "]"
                           for k, v in cases.items()))
        f.write("\n}}\n")
    print(f"{len(cases)} cases, {sum(len(v) for v in cases.values())} launches → {FIXTURE}")
