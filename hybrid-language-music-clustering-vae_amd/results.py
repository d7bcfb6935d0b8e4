"""The consolidated table the three reference scripts share, ``results/clustering_metrics.csv`` (src/Simple_VAE.py:277-294
and its twins in the other two scripts; the column sets are listed in SURVEY.md 5): every script replaces the rows of
its own 'Architecture' and leaves the others' alone."""
from __future__ import annotations

import os

CSV_NAME = "clustering_metrics.csv"


def write_clustering_metrics(results_dir, rows, architecture):
    """Merge ``rows`` (records, or a DataFrame) into ``results_dir/clustering_metrics.csv`` as the reference does: read
    the file if present, drop the rows whose 'Architecture' equals ``architecture``, append the new ones (the union of
    the columns is kept, absent values empty), and write with ``index=False``.  A file that cannot be read -- or has
    no 'Architecture' column -- is replaced by a fresh one holding these rows alone.  Every row gets ``architecture``
    in its 'Architecture' column.  Returns the path written."""
    import pandas as pd  # needed by this table alone: the package imports without it
    new = pd.DataFrame(rows).copy()
    if len(new) == 0:
        raise ValueError("rows is empty")
    new["Architecture"] = architecture
    os.makedirs(results_dir, exist_ok=True)
    path = os.path.join(results_dir, CSV_NAME)
    out = new
    if os.path.exists(path):
        try:
            old = pd.read_csv(path)
            old = old[old["Architecture"] != architecture]
            out = pd.concat([old, new], ignore_index=True)
        except Exception:  # the reference's fallback: an unreadable table is started afresh
            out = new
    out.to_csv(path, index=False)
    return path
