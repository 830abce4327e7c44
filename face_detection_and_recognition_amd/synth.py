"""Deterministic synthetic weights and inputs.

No model weights ship with the reference (GitHub release / Google Drive downloads), and
there is no network, so tests, goldens and the benchmark all run on seeded synthetic weights generated
here from the module's own ``state_dict`` layout.  numpy's PCG64 streams are stable across platforms,
so the same (keys, shapes, seed) reproduce bit-identical tensors in the build container (where the
goldens are made from the reference) and on the GPU box.
Scales are chosen so activations stay O(1) through ~50 layers (otherwise a 1e-4 tolerance is meaningless).
"""
import numpy as np
import torch


def synth_state_dict(template_sd, seed, conv_gain=1.0, residual_gain=None):
    """Fill a state_dict (name -> tensor, only names/shapes are used) with seeded values."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, t in template_sd.items():
        shape = tuple(t.shape)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[name] = torch.zeros(shape, dtype=torch.long)
            continue
        if leaf == "running_mean":
            v = rng.normal(0.0, 0.1, shape)
        elif leaf == "running_var":
            v = rng.uniform(0.8, 1.2, shape)
        elif leaf in ("anchors", "anchor_grid"):
            out[name] = t.clone()
            continue
        elif len(shape) == 4:   # conv weight [O, I/g, kh, kw]
            fan_in = shape[1] * shape[2] * shape[3]
            g = conv_gain
            if residual_gain is not None and ".convs." in name:
                g = residual_gain
            v = rng.normal(0.0, g * np.sqrt(2.0 / fan_in), shape)
        elif len(shape) == 2:   # linear weight [O, I]
            v = rng.normal(0.0, np.sqrt(1.0 / shape[1]), shape)
        elif len(shape) == 1:
            if ".bn" in name or name.startswith("bn.") or ".bn." in name or _is_bn_like(name, template_sd):
                v = rng.uniform(0.8, 1.2, shape) if leaf == "weight" else rng.normal(0.0, 0.1, shape)
            elif "prelu" in name:
                v = rng.uniform(0.1, 0.3, shape)
            elif leaf == "bias":
                v = rng.normal(0.0, 0.05, shape)
            else:
                v = rng.uniform(0.8, 1.2, shape)
        else:
            v = rng.normal(0.0, 1.0, shape)
        out[name] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return out


def _is_bn_like(name, sd):
    """A 1-D 'weight'/'bias' whose sibling 'running_mean' exists belongs to a BatchNorm."""
    prefix = name.rsplit(".", 1)[0]
    return (prefix + ".running_mean") in sd


def synth_frames(n, h, w, seed, blur=8):
    """uint8 [n, h, w, 3] BGR frames: seeded noise, box-blurred so bilinear resize is non-trivial
    (SURVEY 8d), plus two brighter textured patches per frame (the README's two-face video)."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, size=(n, h // blur + 2, w // blur + 2, 3), dtype=np.uint8).astype(np.float32)
    # bilinear-ish upsample by repetition + one smoothing pass (cheap, deterministic)
    up = np.repeat(np.repeat(small, blur, axis=1), blur, axis=2)[:, :h, :w]
    k = blur // 2
    sm = (up + np.roll(up, k, axis=1) + np.roll(up, k, axis=2) + np.roll(np.roll(up, k, axis=1), k, axis=2)) / 4.0
    fine = rng.integers(0, 64, size=(n, h, w, 3), dtype=np.uint8).astype(np.float32)
    out = 0.6 * sm + fine
    return np.clip(out, 0, 255).astype(np.uint8)


def synth_age_gender(net, seed):
    """Seeded weights for an AgeGenderNet (modules/age_gender), in place; returns net.  Every conv / fc weight is
    N(0, 2 / fan_in) (He: the crops' pixel scale, tens after the mean, carries through the ReLUs, so each LRN divides by
    (1 + alpha / 5 * sum x^2)^0.75 of about 1.2 - 2 rather than ~1), biases N(0, 0.05), and fc8 N(0, 0.002^2) so that the
    logits are O(1) and the softmax is not saturated.  The age and the gender net draw different streams."""
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for sub in (net.age, net.gender):
            for name in ("conv1", "conv2", "conv3", "fc6", "fc7", "fc8"):
                p = getattr(sub, name)
                shape = tuple(p.weight.shape)
                fan_in = int(np.prod(shape[1:]))
                std = 0.002 if name == "fc8" else np.sqrt(2.0 / fan_in)
                p.weight.copy_(torch.from_numpy(rng.normal(0.0, std, shape).astype(np.float32)))
                p.bias.copy_(torch.from_numpy(rng.normal(0.0, 0.05, tuple(p.bias.shape)).astype(np.float32)))
    net._plans.clear()
    return net


def _mtcnn_features(sd, pre, x):
    """Calibration only (torch CPU float32): the features in front of the heads of pnet / rnet / onet on x (N, H, W, 3)
    normalised pixels, the way the ports run the nets (spatial axes swapped).  pnet: (N, 32, W', H'); others (N, D)."""
    import torch.nn.functional as F
    cp = lambda i, t: F.prelu(F.conv2d(t, sd[f"{pre}.conv{i}.weight"], sd[f"{pre}.conv{i}.bias"]), sd[f"{pre}.prelu{i}.weight"])
    x = x.permute(0, 3, 2, 1)
    if pre == "pnet":
        return cp(3, cp(2, F.max_pool2d(cp(1, x), 2, 2, ceil_mode=True)))
    x = cp(3, F.max_pool2d(cp(2, F.max_pool2d(cp(1, x), 3, 2, ceil_mode=True)), 3, 2))
    last = 4
    if pre == "onet":
        x = cp(4, F.max_pool2d(x, 2, 2, ceil_mode=True))
        last = 5
    x = F.linear(x.flatten(1), sd[f"{pre}.fc.weight"], sd[f"{pre}.fc.bias"])
    return F.prelu(x, sd[f"{pre}.prelu{last}.weight"])


def synth_mtcnn(net, seed, shares=(0.02, 0.4, 0.5), frame_hw=(160, 224), n_frames=4, frames=None):
    """Seeded weights for an MTCNN (modules/mtcnn), in place; returns net.  Random weights must drive a WORKING cascade, so
    after the He-scaled draw (PReLU slopes U(0.1, 0.4), biases N(0, 0.05)) the heads are calibrated on the CPU against
    synth_frames(n_frames, *frame_hw, seed) (or the uint8 (n, h, w, 3) `frames` given): the face logit difference z1 - z0 of each net gets a standard deviation of 2 and
    the bias that makes `shares[i]` of the calibration inputs pass net.thresholds[i]; box regressions get a standard deviation
    of 0.1 (boxes stay near their cells), landmarks a mean of 0.5 and a standard deviation of 0.15.  The calibration inputs:
    P-Net sees every level of the pyramid (torch's area interpolation stands in for the exact resize), R-Net and O-Net
    see random square cuts of 20 .. 90 pixels (no larger than the frame).  The shares the cascade then really passes differ (its candidates are not
    random squares); the tests check what they need on their own frames."""
    import torch.nn.functional as F
    from .modules.mtcnn.mtcnn import pyramid
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            shape = tuple(p.shape)
            if ".prelu" in name:
                v = rng.uniform(0.1, 0.4, shape)
            elif name.endswith(".bias"):
                v = rng.normal(0.0, 0.05, shape)
            else:
                v = rng.normal(0.0, np.sqrt(2.0 / int(np.prod(shape[1:]))), shape)
            p.copy_(torch.from_numpy(v.astype(np.float32)))
        sd = {k: v.detach().cpu().float() for k, v in net.state_dict().items()}
        if frames is None:
            frames = synth_frames(n_frames, frame_hw[0], frame_hw[1], seed)
        n_frames, frame_hw = frames.shape[0], tuple(frames.shape[1:3])
        frames = torch.from_numpy(np.ascontiguousarray(frames)).float()
        norm = lambda t: (t - 127.5) * 0.0078125
        chw = frames.permute(0, 3, 1, 2)
        feats = {"pnet": [], "rnet": [], "onet": []}
        for s, lh, lw in pyramid(frame_hw[0], frame_hw[1], net.min_face_size, net.factor):
            lvl = torch.round(F.interpolate(chw, size=(lh, lw), mode="area")).permute(0, 2, 3, 1)
            feats["pnet"].append(_mtcnn_features(sd, "pnet", norm(lvl)).permute(0, 2, 3, 1).reshape(-1, 32))
        for pre, size in (("rnet", 24), ("onet", 48)):
            cuts = []
            for _ in range(192):
                f, l = int(rng.integers(n_frames)), int(rng.integers(20, min(90, min(frame_hw)) + 1))
                y, x = int(rng.integers(0, frame_hw[0] - l + 1)), int(rng.integers(0, frame_hw[1] - l + 1))
                cuts.append(torch.round(F.interpolate(chw[f:f + 1, :, y:y + l, x:x + l], size=(size, size), mode="bilinear",
                                                      align_corners=False)))
            feats[pre].append(_mtcnn_features(sd, pre, norm(torch.cat(cuts).permute(0, 2, 3, 1))))
        for i, pre in enumerate(("pnet", "rnet", "onet")):
            x = torch.cat(feats[pre]).double()
            sub = getattr(net, pre)
            flat = lambda p: p.weight.detach().cpu().double().reshape(p.weight.shape[0], -1)
            # class head: std 2 of z1 - z0, then the bias that passes `share`
            w, b = flat(sub.cls), sub.cls.bias.detach().cpu().double()
            d = x @ (w[1] - w[0])
            g = 2.0 / max(float(d.std()), 1e-6)      # (a constant image has no spread to scale)
            w, d = w * g, d * g
            cut_at = float(torch.quantile(d, 1.0 - shares[i]))
            t = net.thresholds[i]
            b[0], b[1] = 0.0, float(np.log(t / (1.0 - t))) - cut_at
            sub.cls.weight.copy_(w.reshape(sub.cls.weight.shape).float())
            sub.cls.bias.copy_(b.float())
            heads = [(sub.reg, 0.0, 0.1)] + ([(sub.lmk, 0.5, 0.15)] if pre == "onet" else [])
            for head, mean, std in heads:
                w = flat(head)
                out = x @ w.T
                w = w * (std / out.std(0).clamp_min(1e-6))[:, None]
                head.weight.copy_(w.reshape(head.weight.shape).float())
                head.bias.copy_((mean - (x @ w.T).mean(0)).float())
    net._invalidate()
    return net
