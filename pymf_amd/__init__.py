"""pymf_amd -- MI355X-native factorize() hot path of nils-werner/pymf.

Drop-in classes for the reference's `pymf.NMF`, `pymf.NMFALS`, `pymf.SNMF`
(pymf/__init__.py:16-43 star-exports them the same way).
"""
from .nmf import NMF          # noqa: F401
from .nmfals import NMFALS    # noqa: F401
from .snmf import SNMF        # noqa: F401
from .nmfnnls import NMFNNLS  # noqa: F401  (SURVEY 8(f) 'next' row 2)
from .bnmf import BNMF        # noqa: F401  (SURVEY 8(f) 'next' row 1)
from .nndsvd import NNDSVD    # noqa: F401  (SURVEY 8(f) 'next' row 4)
from .cnmf import CNMF        # noqa: F401  (convex NMF)
from .kmeans import Kmeans    # noqa: F401  
from .cmeans import Cmeans    # noqa: F401  
from .sivm import SIVM        # noqa: F401  
from .aa import AA            # noqa: F401  
from .svd import SVD          # noqa: F401  
from .pca import PCA          # noqa: F401  
from .svd import pinv         # noqa: F401  (svd.py:27-45)
from .cur import CUR          # noqa: F401  
from .cmd import CMD          # noqa: F401  
from .cursl import CURSL      # noqa: F401  
from .greedy import GREEDY    # noqa: F401  
from .greedycur import GREEDYCUR   # noqa: F401  
from .sivm_cur import SIVM_CUR     # noqa: F401  
from .laesa import LAESA      # noqa: F401  
from .gmap import GMAP        # noqa: F401  
from .sivm_sgreedy import SIVM_SGREEDY   # noqa: F401  
from .sivm_gsat import SIVM_GSAT   # noqa: F401  
from .chnmf import CHNMF      # noqa: F401  
from . import dist            # noqa: F401
from . import distance        # noqa: F401  
from .distance import vq, pdist   # noqa: F401
from .sub import SUB          # noqa: F401  

__all__ = ["NMF", "NMFALS", "SNMF", "NMFNNLS", "BNMF", "NNDSVD", "CNMF", "Kmeans", "Cmeans", "SIVM", "AA", "SVD", "PCA", "CUR", "CMD", "CURSL", "GREEDY", "GREEDYCUR", "SIVM_CUR", "LAESA", "GMAP", "SIVM_SGREEDY", "SIVM_GSAT", "CHNMF", "SUB", "pinv", "dist", "distance", "vq", "pdist"]
__version__ = "0.1.0"
