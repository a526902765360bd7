"""BOP annotation entries from the records of a SceneBatch (host only; nothing here touches the device).

A BOP scene is one physical scene with many images: `scene_camera.json` and `scene_gt.json` are keyed by image, and
`scene_gt_info.json` comes from `ObjectStats.to_bop`.  One image = one view of a batch scene:

    batch.place(view=v, object_to_camera=True)
    cams, o2c = batch.host_cameras(), batch.object_to_camera.cpu().numpy()
    scene_camera[str(v)] = sl.bop.scene_camera_entry((fx, fy, cx, cy), cams[b])
    scene_gt[str(v)] = sl.bop.scene_gt_entries(o2c[b], mesh_to_object, class_indices)
    masks = batch.render(c, object_masks=True).object_masks          # sl.ObjectMasks: mask/ and mask_visib/ of the chunk
    coco["annotations"] += sl.bop.scene_gt_coco_annotations(masks, b, class_indices, image_id=v, first_id=len(coco["annotations"]) + 1)

The camera frame of the renderer is OpenCV's already (x right, y down, z into the picture: the rotation C of
scene.cpp:489-493 maps camera x, y, z to world -y, -z, +x), so no axis is flipped.  Lengths are metres in the records and
millimetres in BOP."""
import numpy as np

MM = 1000.0


def _mat(m, rows, what):
    a = np.asarray(m.detach().cpu().numpy() if hasattr(m, "detach") else m, dtype=np.float64)
    if a.shape == (rows * 4,):
        a = a.reshape(rows, 4)
    if a.shape != (rows, 4):
        raise ValueError("%s must be a %dx4 matrix" % (what, rows))
    return a


def camera_matrix(intrinsics):
    """3x3 K from (fx, fy, cx, cy), or a 3x3 K taken as it is."""
    a = np.asarray(intrinsics, dtype=np.float64)
    if a.shape == (3, 3):
        return a.copy()
    if a.shape != (4,):
        raise ValueError("intrinsics: (fx, fy, cx, cy) or a 3x3 matrix")
    fx, fy, cx, cy = a
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def scene_camera_entry(intrinsics, camera_pose, depth_scale=1.0):
    """One image's entry of scene_camera.json.  `camera_pose`: camera-to-world, 4x4 (Scene.camera_pose, a row of
    SceneBatch.host_cameras()).  cam_R_w2c row-major, cam_t_w2c in millimetres; `depth_scale` is the factor that turns the
    stored depth image into millimetres."""
    c2w = _mat(camera_pose, 4, "camera_pose")
    R = c2w[:3, :3].T                       # rigid: the inverse rotation is the transpose
    t = -R @ c2w[:3, 3]
    return {"cam_K": [float(v) for v in camera_matrix(intrinsics).reshape(-1)],
            "cam_R_w2c": [float(v) for v in R.reshape(-1)],
            "cam_t_w2c": [float(v) for v in t * MM],
            "depth_scale": float(depth_scale)}


def depth_image_scale(z_max):
    """The finest `depth_scale` (millimetres per unit) with which depths up to `z_max` metres fit BOP's uint16 depth image:
    z_max lands on 65535.  Give it to sl.depth_sensor.make_params and to scene_camera_entry alike."""
    return float(z_max) * MM / 65535.0


def scene_gt_entries(object_to_camera, mesh_to_object, class_indices):
    """One image's list of scene_gt.json, in slot order (entry i = the object with instance index i + 1, as
    ObjectStats.to_bop lists them).  `object_to_camera`: [n_objects, 3, 4] (SceneBatch.object_to_camera[b]);
    `mesh_to_object`: [n_objects, 4, 4], one 4x4 for all, or None for models given in the object frame (Mesh.pretransform --
    a pretransform that scales leaves its scale in cam_R_m2c); `class_indices`: obj_id per object.  cam_R_m2c row-major,
    cam_t_m2c in millimetres."""
    o2c = np.asarray(object_to_camera.detach().cpu().numpy() if hasattr(object_to_camera, "detach") else object_to_camera,
                     dtype=np.float64)
    if o2c.ndim != 3 or o2c.shape[1:] != (3, 4):
        raise ValueError("object_to_camera must be [n_objects, 3, 4]")
    n = o2c.shape[0]
    ids = [int(v) for v in class_indices]
    if len(ids) != n:
        raise ValueError("class_indices: one per object")
    if mesh_to_object is None:
        m2o = np.broadcast_to(np.eye(4), (n, 4, 4))
    else:
        m2o = np.asarray(mesh_to_object, dtype=np.float64)
        if m2o.shape == (4, 4):
            m2o = np.broadcast_to(m2o, (n, 4, 4))
        if m2o.shape != (n, 4, 4):
            raise ValueError("mesh_to_object must be [n_objects, 4, 4] or one 4x4 matrix")
    out = []
    for i in range(n):
        m2c = o2c[i] @ m2o[i]
        out.append({"cam_R_m2c": [float(v) for v in m2c[:, :3].reshape(-1)],
                    "cam_t_m2c": [float(v) for v in m2c[:, 3] * MM],
                    "obj_id": ids[i]})
    return out


def scene_gt_coco_annotations(masks, b, class_indices, image_id, first_id=1):
    """One image's annotations of scene_gt_coco.json from an sl.ObjectMasks: one dict per slot 1..S-1 of scene b, in slot order,
    with the keys the BOP toolkit writes -- id (first_id, first_id + 1, ...), image_id, category_id (class_indices[i - 1]),
    iscrowd (always 0), area (= px_count_visib), bbox (= bbox_visib, (x, y, w, h)), segmentation (the VISIBLE mask as
    uncompressed RLE, {"counts", "size": [H, W]}), width, height -- and one key more, `segmentation_all`: the amodal RLE (the
    whole silhouette).  That key is this project's addition; COCO readers ignore it.  Slots that show nothing are listed as
    well (area 0, bbox -1s, segmentation [H * W]), as ObjectStats.to_bop lists them."""
    ids = [int(v) for v in class_indices]
    if len(ids) != masks.n_slots - 1:
        raise ValueError("class_indices: one per object slot 1..S-1")
    one = masks if masks._single else masks[b]
    visib, whole = one.rles("visib"), one.rles("all")
    area = one.stats.px_count_visib.detach().cpu().tolist()
    bbox = one.stats.bbox_visib.detach().cpu().tolist()
    H, W = masks.size
    return [{"id": int(first_id) + i - 1, "image_id": int(image_id), "category_id": ids[i - 1], "iscrowd": 0,
             "area": int(area[i]), "bbox": [int(v) for v in bbox[i]], "segmentation": visib[i - 1],
             "segmentation_all": whole[i - 1], "width": W, "height": H} for i in range(1, masks.n_slots)]
