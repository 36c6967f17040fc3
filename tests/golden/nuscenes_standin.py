"""A small stand-in for the nuScenes devkit for the fixture generator (TEST ONLY): the devkit (`nuscenes`) is not installed
where the fixtures are made, and the reference's datasets/nuscenes_data.py needs only this much of it.  Written from the
devkit's DOCUMENTED behaviour (its schema description and its tutorial's section on reverse indexing), not from its source:

  NuScenes(version, dataroot, verbose)   every table as a list of records under its name (`.instance`, `.sample`, ...), loaded
                                         from <dataroot>/<version>/<table>.json; `.get(table, token)` -> the record
  reverse indexing                       sample_annotation records gain `category_name` (through their instance); sample_data
                                         records gain `sensor_modality` and `channel` (through their calibrated sensor);
                                         sample records gain `data`, channel -> the token of the sample's KEY-FRAME
                                         sample_data record on that channel, and `anns`, the tokens of their annotations
  create_splits_scenes()                 split -> scene names; here the splits of tests/nuscenes_tree.py

Only the nine tables the reference reads are loaded (the devkit also loads attribute, visibility, log and map, which the
tree does not write).  The fixture is pinned on the reference's code over this stand-in, not over the devkit.

Box and LidarPointCloud are not restated at all: data_classes(DC) derives them at generation time from the classes of the
reference's own datasets/data_classes.py (passed in as the loaded module DC) -- that file is the point-cloud class of the
devkit as the reference carries it, so the `rotate`, `translate` and `corners` that run are the reference's."""
import json
import os

TABLES = ("category", "instance", "sample_annotation", "sample", "sample_data", "scene", "sensor", "calibrated_sensor", "ego_pose")


class NuScenes:
    def __init__(self, version="v1.0-mini", dataroot="/data/sets/nuscenes", verbose=True):
        self.version, self.dataroot, self.verbose = version, dataroot, verbose
        self.table_names = list(TABLES)
        self._index = {}
        for name in TABLES:
            with open(os.path.join(dataroot, version, name + ".json")) as f:
                rows = json.load(f)
            setattr(self, name, rows)
            self._index[name] = {r["token"]: i for i, r in enumerate(rows)}
        for record in self.sample_annotation:
            instance = self.get("instance", record["instance_token"])
            record["category_name"] = self.get("category", instance["category_token"])["name"]
        for record in self.sample_data:
            sensor = self.get("sensor", self.get("calibrated_sensor", record["calibrated_sensor_token"])["sensor_token"])
            record["sensor_modality"], record["channel"] = sensor["modality"], sensor["channel"]
        for record in self.sample:
            record["data"], record["anns"] = {}, []
        for record in self.sample_data:
            if record["is_key_frame"]:
                self.get("sample", record["sample_token"])["data"][record["channel"]] = record["token"]
        for record in self.sample_annotation:
            self.get("sample", record["sample_token"])["anns"].append(record["token"])

    def get(self, table_name, token):
        return getattr(self, table_name)[self._index[table_name][token]]


def splits(table):
    """-> create_splits_scenes() over the given split table"""
    def create_splits_scenes(verbose=False):
        return {k: list(v) for k, v in table.items()}
    return create_splits_scenes


def data_classes(DC):
    """-> (LidarPointCloud, Box) over the reference's datasets.data_classes module DC: the devkit's constructor arguments the
    reference passes (Box(..., name=, token=)), the reference's own methods"""
    class LidarPointCloud(DC.PointCloud):
        pass

    class Box(DC.Box):
        def __init__(self, center, size, orientation, label=float("nan"), score=float("nan"),
                     velocity=(float("nan"), float("nan"), float("nan")), name=None, token=None):
            super().__init__(center, size, orientation, label, score, velocity, name)
            self.token = token

    for cls in (LidarPointCloud, Box):            # module-level names: the reference pickles its preloaded frames
        cls.__qualname__ = cls.__name__
        globals()[cls.__name__] = cls
    return LidarPointCloud, Box
