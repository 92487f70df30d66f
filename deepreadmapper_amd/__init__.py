"""deepreadmapper_amd -- MI355X-native drop-in for DeepReadMapper's query hot path:
HNSW-PQ candidate search (faiss_search), fp32-L2 HNSW search on hnswlib indexes (search), and the
Smith-Waterman rerank (post_process_sw_static), implemented as HIP kernels for gfx950 behind the C
ABI in include/drm_hip.h."""
from ._native import DrmError, lib  # noqa: F401  (ImportError if libdrm_hip.so is missing)
from .search import HnswPqIndex, faiss_search, read_index  # noqa: F401
from .flat import HnswFlatIndex, load_flat_index  # noqa: F401  (fp32-L2 hnswlib backend)
from .rerank import (WindowTable, calc_sw_score, calc_sw_scores, post_process_sw_static,  # noqa: F401
                     rerank_arrays, sw_reranker, GenomeTable, extract_fasta_sequence, post_process_sw_dynamic,
                     rerank_dynamic_arrays, embed_windows, l2_rerank_arrays, post_process_l2_static,
                     l2_rerank_dynamic_arrays, post_process_l2_dynamic, sw_align_arrays, sam_cigar,
                     SW_ALIGNMENT_DTYPE, sw_align_affine_arrays, sw_align_affine_clip_arrays, sw_align_region,
                     sam_cigar_region,
                     SW_MD_DTYPE, sw_align_md_arrays, sam_md)

from .pairing import PAIR_RESULT_DTYPE, pair_hits, pair_hits_device, sam_pair_fields  # noqa: F401  (paired-end reads)
from .pairing import (RESCUE_RESULT_DTYPE, mate_rescue, mate_rescue_device, mate_rescue_region,  # noqa: F401
                      mate_rescue_window, pair_rescue_choose)  # (mate rescue)
from .pairing import (TLEN_ESTIMATE_FIELDS, TLEN_SAMPLE_DTYPE, tlen_estimate, tlen_scan,  # noqa: F401
                      tlen_scan_device)  # (the template-length window from the reads)
from .mapq import (MAPQ_RESULT_DTYPE, PAIR_MAPQ_RESULT_DTYPE, hit_mapq, hit_mapq_device, mapq_params,  # noqa: F401
                   mapq_value, pair_mapq, pair_mapq_device, pair_mapq_rescued)  # (mapping quality)
from .loci import LOCI_DROP_DEFAULT, hit_loci, hit_loci_device, loci_params  # noqa: F401  (the locus list of a read)
from .contigs import ContigTable, contig_hits, contig_hits_device, fasta_contigs  # noqa: F401  (multi-contig references)
from .dups import DupSet, dup_end_word, dup_slot, sam_end5  # noqa: F401  (duplicate marking: a first-seen set)
from .sorting import (sam_sort_key, sort_order, sort_order_device, sort_order_workspace, sort_scan_tiles,  # noqa: F401
                      sort_tile)  # (coordinate order: a stable radix sort)
from .bam import (bam_header, bam_record, bgzf_block, bgzf_bound, bgzf_compress, bgzf_compress_device,  # noqa: F401
                  bgzf_eof, bgzf_workspace)  # (BAM output: BGZF on the device, the record encoder)

__version__ = "0.4.0"
from .executor import Comm, MultiIndex, search_rerank  # noqa: F401  (batch executor, multi-GPU, RCCL gather)
from .exact import QUERY_TILE, exact_search_l2, recall_at_k, set_slice_rows  # noqa: F401  (exhaustive scans, recall@k)
from .encoder import Encoder, Preprocessor, Vectorizer, export_encoder  # noqa: F401  (GRU read encoder)
