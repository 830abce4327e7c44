"""FaceGallery, FacePipeline(gallery=...) and the identify_faces_using_reference command line, on the device."""
import os

import numpy as np
import pytest
import torch


def test_pipeline_gallery_default_off():
    import inspect
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    p = inspect.signature(FacePipeline.__init__).parameters
    assert p["gallery"].default is None and p["top_k"].default == 5 and p["identify_tau"].default is None
    assert p["vote"].default == "top1"


@pytest.fixture(scope="module")
def setup(dev):
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.gallery import FaceGallery
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    det = W.build_detector(dev, W.make_frames(8, dev, seed=8), cand_per_frame=48)
    emb = W.build_embedder(dev)
    ref = W.make_reference(64, dev)
    frames = W.make_frames(6, dev, seed=7)
    plain = FacePipeline(det, emb, ref, tau=0.3).step(frames)
    torch.cuda.synchronize()
    n = plain["n_faces"]
    assert n > 3
    labels = torch.arange(n, dtype=torch.int32) % 3
    gal = FaceGallery(plain["emb"], labels, names={0: "ann", 1: "bob", 2: "cy"}, device=dev)
    return W, det, emb, ref, frames, plain, gal


IDENT = ("top_scores", "top_idx", "identity", "identity_score")


@pytest.mark.gpu
def test_pipeline_identifies_its_own_enrolment(dev, setup):
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    W, det, emb, ref, frames, plain, gal = setup
    n = plain["n_faces"]
    out = FacePipeline(det, emb, ref, tau=0.3, gallery=gal, top_k=4).step(frames)
    torch.cuda.synchronize()
    assert out["n_faces"] == n
    assert out["top_scores"].shape == (n, 4) and out["top_idx"].shape == (n, 4) and out["top_idx"].dtype == torch.int32
    assert out["identity"].shape == (n,) and out["identity"].dtype == torch.int32 and out["identity_score"].shape == (n,)
    assert out["top_idx"][:, 0].cpu().tolist() == list(range(n))
    assert out["identity"].cpu().tolist() == [i % 3 for i in range(n)]
    assert (out["identity_score"].cpu() - 1.0).abs().max() < 1e-4
    assert torch.equal(out["identity_score"], out["top_scores"][:, 0])
    # the other keys are untouched by the option
    for k in ("emb", "info", "keep", "best", "arg", "items"):
        assert torch.equal(out[k], plain[k]), k
    # majority vote through the pipeline: the same rows, the kernel's own rule
    maj = FacePipeline(det, emb, ref, gallery=gal, top_k=4, identify_tau=-1.0, vote="majority").step(frames)
    want = gal.identify(plain["emb"], k=4, tau=-1.0, vote="majority")
    assert torch.equal(maj["identity"], want["label"]) and torch.equal(maj["top_idx"], want["top_idx"])
    with pytest.raises(ValueError):
        FacePipeline(det, emb, ref, gallery=gal, vote="nope")


@pytest.mark.gpu
def test_pipeline_without_gallery_is_unchanged(dev, setup):
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    W, det, emb, ref, frames, plain, gal = setup
    a = FacePipeline(det, emb, ref, tau=0.3, gallery=None).step(frames)
    b = FacePipeline(det, emb, ref, tau=0.3).step(frames)
    torch.cuda.synchronize()
    assert list(a.keys()) == list(b.keys()) == list(plain.keys())
    assert not set(IDENT) & set(a)
    for k in a:
        assert (a[k] == b[k]) if not isinstance(a[k], torch.Tensor) else torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("two_streams", [False, True])
def test_pipeline_gallery_overlapped_matches_step(dev, setup, two_streams):
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    W, det, emb, ref, frames, plain, gal = setup
    batches = [W.make_frames(4, dev, seed=s) for s in (11, 12, 13)]
    want = [FacePipeline(det, emb, ref, gallery=gal).step(f, beside=two_streams) for f in batches]
    pipe = FacePipeline(det, emb, ref, gallery=gal, two_streams=two_streams)
    got = []
    for f in batches:
        r = pipe.step_overlapped(f)
        if r is not None:
            got.append(r)
    got.append(pipe.flush())
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for w, r in zip(want, got):
        if "done" in r:
            torch.cuda.current_stream().wait_event(r["done"])
            torch.cuda.synchronize()
        for k in ("emb",) + IDENT:
            assert torch.equal(r[k], w[k]), k


@pytest.mark.gpu
def test_pipeline_gallery_ragged_and_empty(dev, setup):
    from face_detection_and_recognition_amd.frames import RaggedFrames
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    W, det, emb, ref, frames, plain, gal = setup
    pipe = FacePipeline(det, emb, ref, gallery=gal)
    dense = pipe.step(frames)
    same = pipe.step(RaggedFrames.from_list([frames[i] for i in range(frames.shape[0])], dev))
    for k in ("emb",) + IDENT:
        assert torch.equal(same[k], dense[k]), k
    # no faces: empty tensors of the right shapes
    out = dict(n_faces=0, emb=torch.zeros((0, 512), device=dev))
    pipe._add_identity(out)
    assert out["top_scores"].shape == (0, 5) and out["top_idx"].shape == (0, 5) and out["top_idx"].dtype == torch.int32
    assert out["identity"].shape == (0,) and out["identity"].dtype == torch.int32 and out["identity_score"].shape == (0,)


@pytest.mark.gpu
def test_gallery_save_load_add_remove(dev, setup, tmp_path):
    from face_detection_and_recognition_amd.gallery import FaceGallery
    W, det, emb, ref, frames, plain, gal = setup
    path = gal.save(str(tmp_path / "gallery.npz"))
    back = FaceGallery.load(path, device=dev)
    assert torch.equal(back.embeddings, gal.embeddings) and torch.equal(back.labels, gal.labels) and back.names == gal.names
    assert torch.equal(back.ginv, gal.ginv) and torch.equal(back.g3, gal.g3)
    q = plain["emb"]
    a, b = gal.search(q, 3), back.search(q, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # remove: the row is never returned again; add: rebuilt planes, removed rows stay removed
    n = len(back)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[1] = True
    back.remove(mask)
    s, i = back.search(q, 3)
    assert not (i == 1).any() and i[0, 0] == 0
    rng = np.random.default_rng(3)
    extra = rng.normal(0, 1, (200, back.dim)).astype(np.float32)          # crosses a 128-row plane boundary
    back.add(extra, np.full((200,), 9, np.int32), names={9: "new"})
    assert len(back) == n + 200 and back.name_of(9) == "new" and back.name_of(-1) == "unknown"
    s, i = back.search(torch.from_numpy(extra[[150]]).to(dev), 2)
    assert int(i[0, 0]) == n + 150 and abs(float(s[0, 0]) - 1.0) < 1e-5
    s, i = back.search(q, 3)
    assert not (i == 1).any()
    r = back.identify(torch.from_numpy(extra[:4]).to(dev), k=3, tau=0.9)
    assert r["label"].cpu().tolist() == [9] * 4 and r["votes"].cpu().tolist() == [1] * 4
    again = FaceGallery.load(back.save(str(tmp_path / "g2.npz")), device=dev)
    assert torch.equal(again.ginv, back.ginv) and int((again.ginv == 0).sum()) == 1
    with pytest.raises(ValueError):
        FaceGallery(np.zeros((0, 512), np.float32), np.zeros((0,), np.int32), device=dev)
    # features that are no multiple of 32: zero-padded once, same neighbours as fp64
    g100 = rng.normal(0, 1, (50, 100)).astype(np.float32)
    gal100 = FaceGallery(g100, np.arange(50, dtype=np.int32), device=dev)
    s, i = gal100.search(torch.from_numpy(g100[:7]).to(dev), 1)
    assert i[:, 0].cpu().tolist() == list(range(7)) and (s[:, 0].cpu() - 1).abs().max() < 1e-5


@pytest.mark.gpu
def test_gallery_from_feature_files(dev, setup, tmp_path):
    from face_detection_and_recognition_amd.face_extraction import extract_faces_from_dataset as X
    from face_detection_and_recognition_amd.gallery import FaceGallery
    W, det, emb, ref, frames, plain, gal = setup
    e = plain["emb"].cpu().numpy()
    n = e.shape[0]
    half = n // 2
    parts = {"ann": e[:half], "bob": e[half:]}
    c2l = {"ann": 4, "bob": 2}
    for name, rows in parts.items():
        recs = [X.FrameFacesObj(i, 0.0, [0.9] * len(r), [0.5] * len(r), np.zeros((len(r), 4), np.float32), feats=list(r))
                for i, r in enumerate(np.array_split(rows, max(1, (len(rows) + 2) // 3)))]      # <= 3 faces per frame
        X.save_extracted_faces(recs, f"media_{name}", name, str(tmp_path / "feats" / name), 512, c2l)
    g = FaceGallery.from_feature_files(str(tmp_path / "feats"), 512, device=dev)
    assert len(g) == n and g.names == {4: "ann", 2: "bob"}                    # the zero padding rows are gone
    assert np.array_equal(g.embeddings.cpu().numpy(), e)
    assert g.labels.cpu().tolist() == [4] * half + [2] * (n - half)
    one = FaceGallery.from_feature_files([str(tmp_path / "feats" / "bob" / "media_bob.npy")], 512, device=dev)
    assert len(one) == n - half and set(one.labels.cpu().tolist()) == {2}
    with pytest.raises(ValueError):
        FaceGallery.from_feature_files(str(tmp_path / "nothing_here"), 512, device=dev)


@pytest.mark.gpu
def test_identify_faces_using_reference_cli(dev, tmp_path):
    from PIL import Image
    from face_detection_and_recognition_amd.modules.mobile_facenet.mobile_facenet import MobileFaceNet
    from face_detection_and_recognition_amd.similar_face_filtering import identify_faces_using_reference as I
    from face_detection_and_recognition_amd.synth import synth_state_dict
    rng = np.random.default_rng(0)
    net = MobileFaceNet(512)
    net.load_state_dict(synth_state_dict(net.state_dict(), 300))
    wpath = str(tmp_path / "mfn.pth")
    torch.save(net.state_dict(), wpath)
    base = {c: rng.integers(0, 256, (64, 64, 3), dtype=np.uint8) for c in ("class_a", "class_b")}
    for c in base:
        os.makedirs(tmp_path / "ref" / c)
        for i in range(4):
            img = np.clip(base[c].astype(int) + rng.integers(-4, 4, base[c].shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(tmp_path / "ref" / c / f"{c}_{i}.jpg", quality=95)
    os.makedirs(tmp_path / "unl" / "nested")
    copies = {}
    for c in base:                                         # copies of reference images: they must land in their own class
        for i in (0, 2):
            dst = tmp_path / "unl" / ("nested" if i else "") / f"copy_{c}_{i}.jpg"
            dst.write_bytes((tmp_path / "ref" / c / f"{c}_{i}.jpg").read_bytes())
            copies[I.target_name(str(dst), str(tmp_path / "unl"))] = c
    for i in range(5):                                     # seeded noise: wherever the gallery says
        Image.fromarray(rng.integers(0, 256, (48 + 8 * i, 64, 3), dtype=np.uint8)).save(tmp_path / "unl" / f"noise_{i}.jpg", quality=95)
    argv = ["--ud", str(tmp_path / "unl"), "--rd", str(tmp_path / "ref"), "--td", str(tmp_path / "out"), "-m", wpath, "-b", "4",
            "-r", "3", "-k", "3", "--tau", "0.5", "--vote", "majority", "-d", "hip:0"]
    counts = I.main(argv)
    paths = I.unlabelled_images(str(tmp_path / "unl"))
    assert len(paths) == 9 and sum(counts.values()) == 9 and set(counts) == {"class_a", "class_b", "unknown"}
    landed = {f: d for d in counts for f in os.listdir(tmp_path / "out" / d)}
    assert len(landed) == 9
    for f, c in copies.items():
        assert landed[f] == c, f
    # every file where FaceGallery.identify on embed_images of the same files says
    args = I.get_parsed_args(argv)
    model = I.load_model(args)
    gal = I.enrol_reference(model, args.reference_data_path, args)
    assert len(gal) == 6 and gal.names == {0: "class_a", 1: "class_b"}           # -r 3 images per class
    feats = I.embed_images(model, paths, 4, preprocess=args.preprocess)
    lab = gal.identify(feats, k=3, tau=0.5, vote="majority")["label"].cpu().tolist()
    for p, l in zip(paths, lab):
        assert landed[I.target_name(p, str(tmp_path / "unl"))] == gal.name_of(l), p
    assert counts["class_a"] >= 2 and counts["class_b"] >= 2
