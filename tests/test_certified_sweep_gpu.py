"""Round 6: certificate-driven precision for the proposal sweep (object_reasoning.py:301-337,525-557).

  * the device-side argmax certificate (csrc/reasoning.hip::center_peaks_cert_kernel) against the CPU oracle's
    (oracle.peak_certificate, itself pinned to the certificate the fixture generator computed with the reference's own erode / score
    functions, tests/test_oracle_golden_r2.py): same max, same first argmax as the plain peak kernel, same certified set, on the
    reference-made peak fixtures and on perturbed copies of them;
  * soundness, tested directly: for certified maps, random field perturbations just below eps never move the argmax;
  * the certificate-driven sweep (reasoning.sweep_proposals(precision='certified'): three-term products for every proposal, six-term
    re-run of the uncertified ones) returns the SAME peak indices as the full six-term sweep for all 1225 proposals of an image;
  * all 1225 proposals of one 640x480 image against the CPU oracle: every proposal the oracle certifies at eps = 2e-4 must have the
    oracle's peak index (the certificate is what makes 'equal' a theorem rather than luck; uncertified near-ties are reported)."""
import numpy as np
import pytest
import torch

import peaks_common as pc
from oracle import objectness_oracle as orc
from unmore_amd import synth

pytestmark = pytest.mark.gpu
EPS = 2e-4


def _fields(tag, g):
    if tag in pc.SYN:
        B, H, W, seed = pc.SYN[tag]
        return tuple(torch.from_numpy(a) for a in synth.object_like_fields(B, H, W, seed))
    return torch.from_numpy(g[f"{tag}_sdf_maps"]), torch.from_numpy(g[f"{tag}_center_fields"])


@pytest.mark.parametrize("tag", ["syn128", "e2e_base128", "e2e_tiny128"])
def test_device_certificate_equals_the_oracle_certificate(tag):
    from unmore_amd import reasoning
    g = pc.load()
    sdf, cen = _fields(tag, g)
    B = sdf.shape[0]
    # the fixture's maps, plus copies that exercise the other branches: no peak at all (boundary distance pushed negative, centre field
    # shrunk), and a diverging field (negative scores inside a surviving mask)
    sdf_all = torch.cat([sdf, sdf - 5.0, sdf])
    cen_all = torch.cat([cen, cen * 0.1, -cen])
    mx0, am0 = reasoning.center_peaks(sdf_all.cuda(), cen_all.cuda())
    mx, am, ce = reasoning.center_peaks_certified(sdf_all.cuda(), cen_all.cuda(), EPS)
    assert torch.equal(mx0, mx) and torch.equal(am0, am)                       # the certificate does not change what is picked
    amax_o, arg_o, cert_o = orc.peak_certificate(sdf_all, cen_all, EPS, certify_empty=True)
    np.testing.assert_array_equal(am.cpu().numpy(), arg_o.numpy())
    np.testing.assert_allclose(mx.cpu().numpy(), amax_o.numpy(), atol=1e-12, rtol=0)
    np.testing.assert_array_equal(ce.cpu().numpy(), cert_o.numpy())
    # the fixture's own certificate (made with the reference's functions, positive peaks only) on the unperturbed maps
    np.testing.assert_array_equal((ce[:B].cpu().numpy() & (mx[:B].cpu().numpy() > 0)), g[f"{tag}_argmax_certified"][:B].astype(bool))
    assert int(ce[:B].sum()) >= 3 and int(ce[B:2 * B].sum()) >= 1, ce.tolist()     # both branches are exercised
    print(f"{tag}: certified {ce.tolist()}")


@pytest.mark.parametrize("tag", ["syn128", "e2e_base128"])
def test_certified_argmax_survives_perturbations_below_eps(tag):
    """soundness by trial: 40 random perturbations of max-norm 0.98 eps (uniform noise, sign patterns, smooth ramps) never move the
    argmax of a certified map, and never turn a certified empty map into one with a peak"""
    from unmore_amd import reasoning
    g = pc.load()
    sdf, cen = _fields(tag, g)
    sdf_all, cen_all = torch.cat([sdf, sdf - 5.0]).cuda(), torch.cat([cen, cen * 0.1]).cuda()
    mx, am, ce = reasoning.center_peaks_certified(sdf_all, cen_all, EPS)
    assert int(ce.sum()) >= 4
    gen = torch.Generator(device="cuda").manual_seed(3)
    a = 0.98 * EPS
    for t in range(40):
        if t % 3 == 0:
            ds = (torch.rand(sdf_all.shape, device="cuda", generator=gen) * 2 - 1) * a
            dc = (torch.rand(cen_all.shape, device="cuda", generator=gen) * 2 - 1) * a / 2 ** 0.5      # ||dc|| <= a per pixel
        elif t % 3 == 1:
            ds = torch.sign(torch.rand(sdf_all.shape, device="cuda", generator=gen) - 0.5) * a
            dc = torch.sign(torch.rand(cen_all.shape, device="cuda", generator=gen) - 0.5) * a / 2 ** 0.5
        else:
            ramp = torch.linspace(-1, 1, sdf_all.shape[-1], device="cuda")
            ds = (ramp * (1 if t % 2 else -1)).expand_as(sdf_all) * a
            dc = (ramp.flip(0)).expand_as(cen_all) * a / 2 ** 0.5
        mx2, am2 = reasoning.center_peaks(sdf_all + ds, cen_all + dc)
        moved = (am2 != am) & ce
        assert not bool(moved.any()), (t, torch.nonzero(moved).flatten().tolist())


def _sweep_net():
    from argparse import Namespace
    from unmore_amd.objectness_net import ObjectnessNet
    net = ObjectnessNet("cuda:0", 128, "dpt_base", Namespace(use_bg_sdf=True, sdf_activation="tanh"))
    spec = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.peak_edited_state_dict(spec, "base").items()}
    net.load_state_dict(sd, strict=True)
    net = net.to("cuda:0")
    net.set_compute_dtype(torch.float32)
    net.eval()
    for p in net.parameters():
        p.requires_grad = False
    return net, sd


def _anchors():
    import bench
    return torch.from_numpy(bench.anchors(480, 640))


def test_certified_sweep_equals_the_full_precision_sweep_on_every_proposal():
    from unmore_amd import ops, reasoning
    net, _ = _sweep_net()
    props = _anchors()
    assert props.shape[0] == 1225
    image = torch.from_numpy(synth.blob_images(1, 480, 640, seed=1000)[0]).cuda()
    assert ops.get_f32_mode() == "x3"
    mx_f, am_f, d_f = reasoning.sweep_proposals(net, image, props, 50, precision="full")
    info = {}
    mx_c, am_c, d_c = reasoning.sweep_proposals(net, image, props, 50, precision="certified", info=info)
    assert ops.get_f32_mode() == "x3"                                               # the mode is put back
    torch.cuda.synchronize()
    n_peak = int((mx_f > 0).sum())
    print(f"certified sweep: {info}; {n_peak} of 1225 proposals have a peak; max |amax diff| {float((mx_c - mx_f).abs().max()):.2e}; "
          f"max |delta diff| {float((d_c - d_f).abs().max()):.2e}")
    assert n_peak >= 50, "vacuous sweep"
    assert torch.equal(am_c, am_f)                                                  # every peak index, bit for bit
    assert float((mx_c - mx_f).abs().max()) <= 2 ** 0.5 * 1e-4
    assert 0 <= info["rerun"] < 0.5 * info["proposals"], info                      # the certificate carries most of the sweep
    torch.testing.assert_close(d_c, d_f, atol=2e-3, rtol=2e-3)


def test_all_1225_proposals_of_one_image_against_the_cpu_oracle():
    """The whole per-proposal chain -- crop + resize, ObjectnessNet maps (fp32 parity mode), peak picking -- for EVERY anchor of one
    640x480 image against the CPU oracle (object_reasoning.py:109-137,301-337,528-550 restated): the oracle's own certificate at
    eps = 2e-4 says where equality of the peak index is a theorem given the 1e-4 field contract; there it is required, for both the
    full-precision and the certificate-driven sweep.  ~2-3 minutes of CPU time."""
    from unmore_amd import reasoning
    net, sd = _sweep_net()
    props = _anchors()
    image = torch.from_numpy(synth.blob_images(1, 480, 640, seed=1000)[0])
    info = {}
    mx_c, am_c, _ = reasoning.sweep_proposals(net, image.cuda(), props, 50, precision="certified", info=info)
    mx_f, am_f, _ = reasoning.sweep_proposals(net, image.cuda(), props, 50, precision="full")
    am_c, am_f, mx_f = am_c.cpu(), am_f.cpu(), mx_f.cpu()
    import os
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(cores, 16)))      # a 1-GPU box exposes all host cores but grants 16 (bench.py::_host)
    n_cert = n_peak_cert = 0
    mism_unc = []
    worst_field = 0.0
    for i in range(0, 1225, 50):
        crops = orc.crop_resize(image, props[i:i + 50].tolist(), 128)
        with torch.no_grad():
            out = orc.forward(sd, crops, orc.CONFIGS["dpt_base"])
        amax_o, arg_o, cert_o = orc.peak_certificate(out["sdf_maps"][:, 0].contiguous(), out["center_fields"].contiguous(), EPS, certify_empty=True)
        for j in range(len(arg_o)):
            k = i + j
            if bool(cert_o[j]):
                n_cert += 1
                n_peak_cert += int(float(amax_o[j]) > 0)
                assert int(am_f[k]) == int(arg_o[j]), ("full", k, int(am_f[k]), int(arg_o[j]))
                assert int(am_c[k]) == int(arg_o[j]), ("certified", k, int(am_c[k]), int(arg_o[j]))
            elif int(am_f[k]) != int(arg_o[j]):
                mism_unc.append(k)
        if i == 0:
            with torch.no_grad():
                hip = net.get_prediction(crops.cuda())
            worst_field = max(float((hip["sdf_maps"].cpu() - out["sdf_maps"]).abs().max()), float((hip["center_fields"].cpu() - out["center_fields"]).abs().max()))
            assert worst_field < 1e-4
    print(f"1225 proposals vs the CPU oracle: {n_cert} certified by the oracle ({n_peak_cert} of them with a peak), 0 mismatches among them; "
          f"{len(mism_unc)} uncertified near-ties differ {mism_unc[:10]}; sweep {info}; field error of the first batch {worst_field:.2e}")
    assert n_cert >= 1000 and n_peak_cert >= 20


def test_certified_sweep_decides_like_the_full_sweep_at_a_threshold_beside_a_maximum():
    """The certificate proves `max` stays on its side of the threshold it is GIVEN.  Put the caller's threshold half a certificate bound
    above the full-precision maximum of a proposal that the default threshold certifies: the sweep must re-run that proposal (its
    three-term maximum is within sqrt(2) * 1e-4 of the full one, so within the bound of the threshold) and every decision
    `max > thres` must be the full-precision one -- at that threshold and at the default."""
    from unmore_amd import ops, reasoning
    net, _ = _sweep_net()
    props = _anchors()
    assert props.shape[0] == 1225
    image = torch.from_numpy(synth.blob_images(1, 480, 640, seed=1000)[0]).cuda()
    assert ops.get_f32_mode() == "x3"
    mx_f, am_f, _ = reasoning.sweep_proposals(net, image, props, 50, precision="full")
    info0 = {}
    mx_0, am_0, _ = reasoning.sweep_proposals(net, image, props, 50, precision="certified", info=info0)
    torch.cuda.synchronize()
    assert info0["rerun_indices"] == sorted(info0["rerun_indices"]) and len(info0["rerun_indices"]) == info0["rerun"]
    assert torch.equal(mx_0 > 0.009, mx_f > 0.009)                                   # decisions at the default threshold
    assert torch.equal(am_0, am_f)
    mx_full = mx_f.cpu().numpy()
    rerun0 = set(info0["rerun_indices"])
    cand = [i for i in range(1225) if mx_full[i] > 0 and i not in rerun0]
    assert cand, "vacuous: no proposal with a positive peak is certified at the default threshold"
    cand.sort(key=lambda i: (mx_full[i], i))
    k = cand[len(cand) // 2]                                                          # the median full-precision maximum
    bound = 2 * 2 ** 0.5 * reasoning.CERT_EPS
    thres = float(mx_full[k] + 0.5 * bound)
    info = {}
    mx_c, am_c, _ = reasoning.sweep_proposals(net, image, props, 50, precision="certified", info=info, singular_threshold=thres)
    torch.cuda.synchronize()
    print(f"certified sweep beside a maximum: proposal {k}, full max {mx_full[k]:.6f}, thres {thres:.6f}; default {info0['rerun']} re-run, "
          f"here {info['rerun']}; decisions differ at {int(((mx_c > thres) != (mx_f > thres)).sum())} of 1225")
    assert k in info["rerun_indices"], (k, info["rerun"])
    assert torch.equal(mx_c > thres, mx_f > thres)
    assert torch.equal(am_c, am_f)
