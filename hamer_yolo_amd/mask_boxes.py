"""Hand boxes from label masks, with the detector's pass protocol: the box source of the batched mask-driven folder driver
(``infer.process_batch_manopara_with_mask(..., batched=True)``; reference: hamer/infer.py:1040-1072, ``get_bbox_from_npy``, and
the loop around it, :1099-1220).

``iter_folder_results`` uses a ``MaskBoxes`` where it uses a ``Detector``: ``detect_frames_enqueue`` / ``detect_frames_finish``
per pass of equally sized frames, on the detector's stream.  A pass's masks go up from page-locked memory in one copy, ONE
``hm_mask_boxes`` launch (csrc/mask_boxes.hip) boxes every (frame, requested label), and the ``[Q][5]`` result comes back with
the pass's one host sync.  No pixel of a mask is looked at on the host, except in a mask that has another shape than its frame
(or is no two-dimensional integer / bool array): that file alone is boxed by the host rule of ``get_bbox_from_npy`` and never
shares the batched call.  Such masks are rare -- a mask is a label image OF its frame.

The masks themselves are read by the driver's decode threads (``prefetch``, called behind each frame's decode) into a ring of
page-locked slots that mirrors the driver's ring of frame slots: a uint8 ``.npy`` with one ``readinto`` straight into its slot,
any other integer / bool mask through ``np.load`` and one converting copy.  A pass's masks then lie next to each other and go
up as one slice, with no gathering on the enqueueing thread (gathering 16 + 48 masks there cost 10 of a 64-frame folder's 49
ms).  A slot carries the event behind the last upload that read it, and a decode thread waits for it
before it rewrites the slot.  A mask file that is missing gives the warning ``get_bbox_from_npy`` prints and no result for that frame;
one that cannot be read is reported and treated the same way.
"""
from __future__ import annotations

import os
import threading
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch


def load_label_mask(path: str) -> Optional[np.ndarray]:
    """The label image at ``path`` as it is stored (``allow_pickle=False``); None, with get_bbox_from_npy's warning, when the file
    is missing, and with a message when it cannot be read."""
    if not os.path.exists(path):
        print(f"[Warning] mask not found: {path}")
        return None
    try:
        return np.load(path, allow_pickle=False)
    except Exception as e:
        print(f"[Warning] mask not readable: {path}: {e}")
        return None


def read_bytes_into(path: str, dest: np.ndarray) -> bool:
    """Read the ``.npy`` file at ``path`` straight into ``dest`` when it holds exactly such an array -- uint8, C order, ``dest``'s
    shape -- with one ``readinto`` and no array in between; False (``dest`` may then hold anything) for every other file."""
    try:
        with open(path, "rb", buffering=0) as f:
            version = np.lib.format.read_magic(f)
            if version == (1, 0):
                shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
            elif version == (2, 0):
                shape, fortran, dtype = np.lib.format.read_array_header_2_0(f)
            else:
                return False
            if dtype != np.uint8 or fortran or tuple(shape) != tuple(dest.shape) or not dest.flags.c_contiguous:
                return False
            view, n = memoryview(dest.reshape(-1)), 0
            while n < len(view):
                k = f.readinto(view[n:])
                if not k:
                    return False
                n += k
            return True
    except Exception:
        return False


def as_label_bytes(m: np.ndarray) -> np.ndarray:
    """An integer or bool label image of any width as uint8, by the rule of ``evaluate_masks._load_mask``: what does not fit a
    byte is no label (it becomes 0)."""
    if m.dtype == np.uint8:
        return m
    if m.dtype.kind == "b":
        return m.astype(np.uint8)
    return np.where((m >= 0) & (m <= 255), m, 0).astype(np.uint8)


def host_box(mask: np.ndarray, label: int) -> Optional[List[float]]:
    """get_bbox_from_npy's rule on a loaded mask: [x1, y1, x2, y2] as floats, None when the label is absent."""
    rows, cols = np.where(mask == label)
    if len(rows) == 0:
        return None
    return [float(np.min(cols)), float(np.min(rows)), float(np.max(cols)), float(np.max(rows))]


class MaskBoxes:
    """``MaskBoxes(mask_folder, right_label=3, left_label=None)``: per frame the tight box of ``right_label`` in
    ``<mask_folder>/<stem>.npy`` as a ``'right'`` detection -- the reference's rule: label 3, always a right hand -- and, with
    ``left_label=L``, the box of label L as a ``'left'`` one (for masks that tell the hands apart: the only way such a mask can
    carry a left hand at all).  Labels are 0..255 (``ValueError`` otherwise); wider masks are read by ``as_label_bytes``.

    ``wants_paths`` tells ``iter_folder_results`` to pass the pass's file paths (``paths=``) and to call ``prefetch(path,
    (H, W))`` from its decode threads.  ``labelled`` collects the paths of frames in which a requested label exists, whether or not
    its box has an area: the driver writes the reference's empty record for those that yield no hand."""
    wants_paths = True

    def __init__(self, mask_folder: str, right_label: int = 3, left_label: Optional[int] = None):
        self.mask_folder = str(mask_folder)
        self.sides: List[Tuple[str, int]] = []
        for side, label in (("right", right_label), ("left", left_label)):
            if label is None:
                continue
            if isinstance(label, bool) or int(label) != label or not 0 <= int(label) <= 255:
                raise ValueError(f"MaskBoxes: {side}_label must be an integer in 0..255, got {label!r}")
            self.sides.append((side, int(label)))
        if not self.sides:
            raise ValueError("MaskBoxes: no label requested")
        self.labelled: List[str] = []
        self._loaded: Dict[str, object] = {}
        self._lock = threading.Lock()
        self._ring = None                       # (hw, slots, tensor (slots, H, W) uint8 page-locked, its numpy view)
        self._slot_events: Dict[int, object] = {}

    # ------------------------------------------------------------------ host side
    def mask_path(self, image_path: str) -> str:
        return os.path.join(self.mask_folder, os.path.splitext(os.path.basename(image_path))[0] + ".npy")

    def queries(self, frames) -> List[Tuple[int, int]]:
        """One (frame, label) query per frame of the batched call and requested label, frame-major, right before left.
        ``frames``: how many (0 .. n-1), or the frames' places in the uploaded batch."""
        return [(f, label) for f in (range(frames) if isinstance(frames, int) else frames) for _, label in self.sides]

    def _slot(self, hw, slot, slots):
        """The numpy view of page-locked slot ``slot`` of ``slots`` for masks of ``hw``, safe to write (the upload that last read
        it has finished), or None: the ring serves the folder's first frame size only."""
        if slot is None or not slots:
            return None
        with self._lock:
            if self._ring is None:
                t = torch.empty((int(slots),) + tuple(hw), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
                self._ring = (tuple(hw), int(slots), t, t.numpy())
            ring = self._ring
        if ring[0] != tuple(hw) or ring[1] != int(slots):
            return None
        ev = self._slot_events.get(slot)
        if ev is not None:
            ev.synchronize()
        return ring[3][slot]

    def _load(self, image_path: str, hw, dest: Optional[np.ndarray] = None) -> object:
        """None (no mask), a (H, W) uint8 array for the batched call -- ``dest`` itself, filled, when one is given --, or
        ``("host", detections)`` for a mask that cannot share it: another shape than its frame, or no 2-D integer / bool array."""
        path = self.mask_path(image_path)
        if dest is not None and os.path.exists(path) and read_bytes_into(path, dest):
            return dest
        m = load_label_mask(path)
        if m is None:
            return None
        if m.ndim == 2 and tuple(m.shape) == tuple(hw) and m.dtype.kind in "uib":
            if dest is None:
                return np.ascontiguousarray(as_label_bytes(m))
            np.copyto(dest, as_label_bytes(m))
            return dest
        try:
            boxes = [(side, host_box(m, label)) for side, label in self.sides]
        except Exception as e:
            print(f"[Warning] mask not usable: {path}: {e}")
            return None
        return ("host", [[side, b] for side, b in boxes if b is not None])

    def prefetch(self, image_path: str, hw, slot: Optional[int] = None, slots: int = 0) -> None:
        """Read the frame's mask now (a decode thread calls this); the pass that holds the frame takes it from memory.  With
        ``slot`` / ``slots`` -- the frame's place in the driver's ring of page-locked frame slots and the ring's size -- the mask
        is read straight into the same place of a page-locked ring of masks, so that a pass's masks lie next to each other and
        go up in one copy without being gathered first."""
        dest = self._slot(hw, slot, slots)
        got = self._load(image_path, hw, dest)
        with self._lock:
            self._loaded[image_path] = (tuple(hw), got, slot if (dest is not None and got is dest) else None)

    def _take(self, image_path: str, hw):
        """(what ``_load`` gave, the mask's slot in the page-locked ring or None)."""
        with self._lock:
            hit = self._loaded.pop(image_path, None)
        if hit is not None and hit[0] == tuple(hw):
            return hit[1], hit[2]
        return self._load(image_path, hw), None

    def _detections(self, rows) -> Tuple[List, bool]:
        """The [Q / frame][5] rows of one frame -> (detection list, does a requested label exist)."""
        dets, found = [], False
        for (side, _), (x1, y1, x2, y2, n) in zip(self.sides, rows):
            if n > 0:
                found = True
                dets.append([side, [float(x1), float(y1), float(x2), float(y2)]])
        return dets, found

    # ------------------------------------------------------------------ the detector's pass protocol
    def detect_frames_enqueue(self, frames, paths=None):
        """Upload the masks of ``frames`` (equally sized (H, W, 3) device frames; ``paths``: their image files) in one copy from
        page-locked memory and box them with one hm_mask_boxes launch on the current stream; the result is copied into
        page-locked memory of THIS call.  No host sync."""
        if paths is None or len(paths) != len(frames):
            raise ValueError("MaskBoxes.detect_frames_enqueue needs the pass's file paths (paths=[...], one per frame)")
        hw = (int(frames[0].shape[0]), int(frames[0].shape[1]))
        taken = [self._take(p, hw) for p in paths]
        got = [g for g, _ in taken]
        rows_of = [i for i, g in enumerate(got) if isinstance(g, np.ndarray)]
        rows, ev = (None, None)
        if rows_of:
            rows, ev = self._boxes_enqueue([got[i] for i in rows_of], hw, frames[0].device, slots=[taken[i][1] for i in rows_of])
        return {"paths": list(paths), "got": got, "rows_of": rows_of, "rows": rows, "event": ev}

    def _boxes_enqueue(self, masks: List[np.ndarray], hw, dev, slots=None):
        """The device step of a pass: ``masks`` ((H, W) uint8 arrays; ``slots``: their places in the page-locked ring, or None) ->
        (the [Q][5] rows in page-locked memory, the event behind their copy).  Masks that lie in ascending ring slots go up as
        the ONE slice that spans them (a frame without a mask leaves a gap that no query names); otherwise -- the pass wraps
        round the ring, a mask was loaded late -- they are gathered into page-locked memory of this call first.  The library
        has no CPU form of this step; the host-only tests of the driver's bookkeeping replace this method."""
        from .hamer.utils import mask_eval as ME
        in_ring = bool(slots) and all(s is not None for s in slots) and all(a < b for a, b in zip(slots, slots[1:]))
        if in_ring:
            lo, hi = slots[0], slots[-1]
            dev_masks = self._ring[2][lo:hi + 1].to(dev, non_blocking=True)
            up = torch.cuda.Event()
            up.record()
            for s in range(lo, hi + 1):
                self._slot_events[s] = up
            places = [s - lo for s in slots]
        else:
            stage = torch.empty((len(masks),) + tuple(hw), dtype=torch.uint8, pin_memory=True)
            view = stage.numpy()
            for j, m in enumerate(masks):
                np.copyto(view[j], m)
            dev_masks = stage.to(dev, non_blocking=True)
            places = len(masks)
        qd = torch.from_numpy(ME.box_query_table(self.queries(places))).pin_memory().to(dev, non_blocking=True)
        boxes = ME.mask_boxes(dev_masks, qd)
        rows = torch.empty(tuple(boxes.shape), dtype=torch.int32, pin_memory=True)
        rows.copy_(boxes, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return rows, ev

    def detect_frames_finish(self, token):
        """Wait for that pass (its event only) and return ``(None, dets_lists)``: per frame ``[['right', [x1, y1, x2, y2]], ...]``
        with float coordinates, as ``get_bbox_from_npy`` gives them; an empty list where the mask or the label is missing."""
        if token["event"] is not None:
            token["event"].synchronize()
        rows = token["rows"]
        return None, self._collect(token["paths"], token["got"], token["rows_of"], rows.numpy() if torch.is_tensor(rows) else rows)

    def _collect(self, paths, got, rows_of, boxes) -> List[List]:
        k = len(self.sides)
        place = {i: j for j, i in enumerate(rows_of)}
        out = []
        for i, (p, g) in enumerate(zip(paths, got)):
            if g is None:
                out.append([])
                continue
            if i in place:
                dets, found = self._detections(boxes[place[i] * k:(place[i] + 1) * k].tolist())
            else:
                dets, found = g[1], bool(g[1])
            if found:
                self.labelled.append(p)
            out.append(dets)
        return out
